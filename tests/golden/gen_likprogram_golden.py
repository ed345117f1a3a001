#!/usr/bin/env python
"""Golden vectors of the likelihood-program tests: the reference itself fitted with bl.om.SymPy Normal (two parameters), Poisson (one) and
Frechet (three), the studies of tests/likprogram_studies.py.  Imports the reference (build container only; BAYESLOOP_REFERENCE names its
checkout); writes tests/golden/likprogram_*.npz -- data only.
    python tests/golden/gen_likprogram_golden.py"""
import math
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
warnings.filterwarnings('ignore')
np.math = math
sys.path.insert(0, os.environ.get('BAYESLOOP_REFERENCE', '/root/reference'))
import bayesloop as bl              # noqa: E402  (the reference)
import likprogram_studies as ls     # noqa: E402

for name, make in ls.GOLDEN.items():
    S = make(bl)
    S.fit(silent=True)
    np.savez_compressed(os.path.join(HERE, name + '.npz'), **ls.results(S))
    print('%-24s logE = %.12f' % (name, S.logEvidence))
