"""CPU: the floor of the bar of tests/test_gpu_ipma.py.  Per case of tests/helpers_ipma.py and per set of bounds, on the oracle's fits of the nine resamples
of the test and of all rows: per field the largest |fp64 mirror - longdouble mirror| (plspm.ipma._ipma), the smallest |weight_r_p|, whether the full sample is
admissible and how many of the nine replicates are.

    python tools/ipma_floor.py [case ...]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("plspm-python_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, sub))
from helpers_ipma import CASES, case, field_difference, mirror_pair, observed_bounds, oracle_record, resamples, wider_bounds  # noqa: E402
from plspm.ipma import FIELDS  # noqa: E402

for name in (sys.argv[1:] or CASES):
    X, model, _, _, _ = case(name)
    idx = resamples(X, 9)
    records = [oracle_record(X, model, rows) for rows in [None] + list(idx)]
    for label, bounds in (("observed", observed_bounds), ("wider", wider_bounds)):
        lo, hi = bounds(X, model)
        worst, smallest, status = {f: 0.0 for f in FIELDS}, float("inf"), []
        for rows, (rec, pairs) in zip([None] + list(idx), records):
            Xr = (X if rows is None else X[rows])[:, model.mv_order]
            m64, mld = mirror_pair(Xr, model, rec, pairs, lo, hi)
            for f, d in field_difference(m64, mld).items():
                worst[f] = max(worst[f], d)
            smallest = min(smallest, m64["min_abs_weight"])
            status.append(m64["status"])
        print("%-12s %-8s %s   min |weight_r| %.1e   full sample status %d, %d of 9 replicates admissible"
              % (name, label, "  ".join("%s %.1e" % (f, worst[f]) for f in FIELDS), smallest, status[0], sum(s == 0 for s in status[1:])))
