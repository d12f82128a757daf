"""Writes tests/golden/norm_bounds.json: per case and quantity of
tests/_norm_cases.py, 8 x the largest |float32 restatement - float64| (the
reference's order of operations, left-to-right sums), floored at 4 ulp of the
quantity's largest magnitude; the same for three training iterations of the tiny
net of tests/test_gpu_norm_layers.py ("tiny_net") and for a BatchNorm that sits
on the data blob ("bn_on_data").  The GPU tests read the file; nothing in it
comes from the kernels under test.  Also records, for case (b) (inputs
100 + 0.1 z), that a float32 one-pass E[x^2] - E[x]^2 restatement breaks the
bound of rstd and xhat while the two-pass restatement holds it.

    python tests/golden/make_norm_bounds.py
"""
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import _norm_cases as nc  # noqa: E402


def main():
    out = {"rule": "max(8 * max|f32 restatement - f64|, 4 ulp32(max|f64|))", "cases": {}}
    for name in nc.BN_CASES:
        q32, q64 = nc.quantities(name, np.float32), nc.quantities(name, np.float64)
        out["cases"][name] = {k: nc.bound(q32[k], q64[k]) for k in q64}
    # (b)'s folded quantities are left out: at 100 + 0.1 z the float32 restatement's ReLU mask differs from
    # float64's on outputs next to 0, which makes their bounds meaningless; the fold is checked on the other cases
    for k in ("y_fold", "dx_fold", "dx_global", "dgamma", "dbeta"):
        del out["cases"]["b"][k]
    # the tiny net of tests/test_gpu_norm_layers.py: three momentum-SGD iterations
    t32, t64 = nc.tiny_train(np.float32), nc.tiny_train(np.float64)
    out["tiny_net"] = [dict(loss=nc.bound(a["loss"], b["loss"]),
                            grads={k: nc.bound(a["grads"][k], b["grads"][k]) for k in b["grads"]},
                            params={k: nc.bound(a["params"][k], b["params"][k]) for k in b["params"]})
                       for a, b in zip(t32, t64)]
    d32, d64 = nc.bn_on_data(np.float32)[1], nc.bn_on_data(np.float64)[1]
    out["bn_on_data"] = {k: nc.bound(d32[k], d64[k]) for k in d64}
    _, _, e32 = nc.running_sequence(np.float32)
    _, _, e64 = nc.running_sequence(np.float64)
    out["cases"]["e"] = {k: nc.bound(e32[k], e64[k]) for k in e64}
    x, dy = nc.sigmoid_inputs()
    s32, s64 = nc.sigmoid(x, dy, np.float32), nc.sigmoid(x, dy, np.float64)
    out["cases"]["sigmoid"] = {"y": nc.bound(s32[0], s64[0]), "dx": nc.bound(s32[1], s64[1])}
    # (b): one pass against two passes, both in float32, against the bound
    q64, two, one = (nc.quantities("b", np.float64), nc.quantities("b", np.float32),
                     nc.quantities("b", np.float32, one_pass=True))
    rec = {}
    for k in ("rstd", "xhat"):
        err = lambda q: float(np.max(np.abs(q[k].astype(np.float64) - q64[k])))  # noqa: E731
        rec[k] = {"bound": out["cases"]["b"][k], "two_pass_error": err(two), "one_pass_error": err(one)}
        assert rec[k]["two_pass_error"] <= rec[k]["bound"] < rec[k]["one_pass_error"], (k, rec[k])
    out["one_pass_check_b"] = rec
    (HERE / "norm_bounds.json").write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
