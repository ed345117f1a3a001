#!/usr/bin/env python
"""
Generates the fixtures of tests/chain_nd_cases.py (chain batches on grids with three parameters: a 16-chain hyper-study with two
walks, a change-point study over 16 candidates; 5 x 18 x 14 cells) under tests/golden/ by IMPORTING THE REFERENCE, exactly as
gen_golden.py does (same two shims).  The change-point study keeps a subset of its posterior rows (store = 'sparse').  CPU only.
Run:  python tests/golden/gen_chain_nd_golden.py [case ...]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden             # noqa: E402  (installs the shims, imports the reference as gen_golden.bl)
import gen_combined_golden    # noqa: E402  (run: gen_golden.run for a spec dict)
import chain_nd_cases as cn   # noqa: E402


def main():
    for name in sys.argv[1:] or cn.GOLDEN:
        out = gen_combined_golden.run(cn.ND[name])
        path = os.path.join(HERE, name + '.npz')
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        assert size < 200_000, (name, size)
        print('%-34s logE=%r  %6.1f kB' % (name, float(out['logEvidence']), size / 1e3), flush=True)


if __name__ == '__main__':
    main()
