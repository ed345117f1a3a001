#!/usr/bin/env python
"""
Generates the fixtures of tests/nd_transition_cases.py (NotEqual, Independent, Serial and Deterministic models on grids with three and
four parameters) under tests/golden/ by IMPORTING THE REFERENCE, exactly as gen_golden.py does (same two shims).  CPU only.
Run:  python tests/golden/gen_nd_transition_golden.py [case ...]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden             # noqa: E402  (installs the shims, imports the reference as gen_golden.bl)
import gen_combined_golden    # noqa: E402  (run: gen_golden.run for a spec dict)
import cases                  # noqa: E402
import nd_transition_cases as ndc   # noqa: E402


def main():
    names = sys.argv[1:] or (ndc.GOLDEN + ndc.GOLDEN_ONLINE)
    for name in names:
        if name in ndc.ONLINE:
            cases.ONLINE_CASES.setdefault(name, ndc.ONLINE[name])      # (gen_golden.run_online looks the spec up there; this process only)
            out = gen_golden.run_online(name)
        else:
            out = gen_combined_golden.run(ndc.ND[name])
        path = os.path.join(HERE, name + '.npz')
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        assert size < 200_000, (name, size)
        print('%-34s logE=%r  %6.1f kB' % (name, float(out['logEvidence']), size / 1e3), flush=True)


if __name__ == '__main__':
    main()
