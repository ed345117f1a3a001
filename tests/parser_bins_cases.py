"""The studies, queries and maps of the distribution-query tests (tests/test_parser_bins_host.py, tests/test_parser_bins.py) and of the
generator of their fixtures (tests/golden/gen_parser_bins_golden.py), and a NumPy restatement of the order in which the device adds the
cells of a bin (bayesloop_amd/csrc/blhip_bins.hpp), written from the header's description:

* the cells are cut into slabs of `slab`; inside a slab the cells with a bin are ordered stably by bin -- a RUN is the cells of one bin
  in one slab, in ascending cell order;
* a run is cut into GROUPS of `gw` cells (the last one padded with zeros); a group is added from its first cell to its last, starting
  from 0.0; the groups of a run are added in ascending order, starting from the first group's sum;
* the runs of a bin are added in ascending slab order, starting from 0.0.
gw is the group width the library chooses for the map: 1 if every run is one cell, else the power of two >= the mean run length, at
least 2 and at most the width asked for."""
import numpy as np

import parser_series_cases as psc

BUILDERS = psc.BUILDERS

# builder -> queries without a relation; every one is a one-space query over the parameters of the builder's only study
QUERIES = {
    'gauss': ('mean/std', 'mean + std', 'std^2', 'log(mean)', 'sqrt(mean)*std', 'mean*std'),
    'coal': ('accident_rate*2', 'accident_rate^2', 'log(accident_rate)'),
    'hyper_alone': ('mean/std', 'mean + std', 'std^2'),
}
# (builder, query) -> (n_bins of the scalar path, cells in the smallest bin that has any, in the largest, cells left out); None: not pinned
FIGURES = {
    ('gauss', 'mean/std'): (22, 1, 230, 1), ('gauss', 'mean + std'): (60, 1, 12, 1), ('gauss', 'std^2'): (10, 24, 144, 24),
    ('gauss', 'log(mean)'): (2, 340, 340, 140), ('gauss', 'sqrt(mean)*std'): (33, 1, 23, 121),
    ('coal', 'accident_rate*2'): (198, 1, 2, None), ('coal', 'accident_rate^2'): (100, 1, 20, None), ('coal', 'log(accident_rate)'): (7, 2, 117, None),
}
GAUSS_NAN = {'log(mean)': 120}           # cells of 'gauss' whose value is NaN
# (a query that is one function call, 'log(mean)', trips the reference's own evaluator -- parser.py:167, IndexError -- so the case with NaNs is the root)
REFERENCE_CASES = (('gauss', 'mean/std'), ('gauss', 'sqrt(mean)*std'), ('coal', 'accident_rate^2'))
PARENT_STAMP_INDICES = (0, 7, -1)
# queries the scalar call raises on (and so does the loop): n_bins = 1 -> IndexError; a constant derived value -> int(nan): ValueError
RAISING = (('coal', '1/accident_rate', IndexError), ('coal', 'accident_rate*0', ValueError))


def key(builder, query):
    return builder + '|' + query


def figures(index, ok, n_bins):
    """(n_bins, smallest occupied bin, largest bin, cells left out) of a scalar-path binning"""
    counts = np.bincount(index[ok], minlength=max(n_bins - 1, 1))
    return int(n_bins), int(counts[counts > 0].min()), int(counts.max()), int((~ok).sum())


# ---- the order of the device's additions ------------------------------------------------------------------------------------------------
def group_width(bin_map, slab, gw_max):
    bin_map = np.asarray(bin_map)
    runs = cells = 0
    for lo in range(0, bin_map.size, slab):
        b = bin_map[lo:lo + slab]
        b = b[b >= 0]
        runs += np.unique(b).size
        cells += b.size
    if runs == 0 or cells == runs:
        return 1
    gw = 2
    while gw < gw_max and gw * runs < cells:
        gw *= 2
    return gw


def runs_of(bin_map, slab):
    """[(slab index, bin, cells of the run in ascending order)] in the order of the library's run numbers: by slab, then by bin"""
    bin_map = np.asarray(bin_map)
    out = []
    for k, lo in enumerate(range(0, bin_map.size, slab)):
        b = bin_map[lo:lo + slab]
        for v in np.unique(b[b >= 0]):
            out.append((k, int(v), lo + np.nonzero(b == v)[0]))
    return out


def kernel_order_sums(rows, bin_map, n_bins, slab, gw):
    """(len(rows), n_bins) float64: rows[s][c] added over the cells of every bin in the device's order, one IEEE addition at a time"""
    rows = np.asarray(rows, dtype=np.float64)
    out = np.zeros((rows.shape[0], n_bins))
    for _, b, cells in runs_of(bin_map, slab):
        run = None
        for g0 in range(0, len(cells), gw):
            acc = np.zeros(rows.shape[0])
            for c in cells[g0:g0 + gw]:
                acc = acc + rows[:, c]
            run = acc if run is None else run + acc
        out[:, b] = out[:, b] + run
    return out


# ---- maps for the kernel tests: name -> (G, n_bins, map) given the slab length -------------------------------------------------------------
def maps(slab):
    rs = np.random.RandomState(11)
    out = {}

    def put(name, n_bins, m):
        m = np.asarray(m, dtype=np.int32)
        assert m.min() >= -1 and m.max() < n_bins
        out[name] = (m.size, n_bins, m)

    put('one-cell', 1, [0])
    for G in (255, 256, 257):
        put('G%d-2bins' % G, 2, np.arange(G) % 3 - 1)                       # a third of the cells left out
    for nb in (63, 64, 65):
        put('%dbins' % nb, nb, rs.randint(-1, nb, size=300))
    put('more-bins-than-threads', 700, rs.permutation(np.arange(slab + 1) % 700))      # one slab plus one cell
    put('own-bin', 257, np.arange(257)[::-1])                               # n_bins == G, every cell its own bin
    put('one-bin', 1, np.zeros(2 * slab + 77, dtype=int))                   # three slabs, the last one partial
    put('all-out', 5, -np.ones(slab + 1, dtype=int))
    seam = np.full(2 * slab + 9, 3)
    seam[:slab - 40] = rs.randint(0, 3, size=slab - 40)                     # bin 3: the last 40 cells of slab 0 and on through slab 1 into slab 2
    put('seam', 4, seam)
    ends = rs.randint(0, 6, size=2 * slab + slab // 2 + 2)
    ends[ends == 2] = 3
    ends[[5, 6, slab - 1, 2 * slab + 1, ends.size - 1]] = 2                 # bin 2 in the first and last slab only
    assert not (ends[slab:2 * slab] == 2).any()
    put('first-and-last', 6, ends)
    G = 2 * slab + 101
    skew = np.empty(G, dtype=int)
    half = rs.permutation(G)[:G // 2]
    skew[:] = -2
    skew[half] = 0                                                          # one bin with half the cells, the rest singletons
    skew[skew == -2] = 1 + np.arange((skew == -2).sum())
    put('skewed', int(skew.max()) + 1, skew)
    return out


def row_families(G, T, seed):
    """'tiny': values from 1 down to 1e-300 with exact zeros; 'exact': multiples of 2^-30 below 2^10 -- a sum of up to 2^12 of them is exact in
    any order"""
    rs = np.random.RandomState(seed)
    tiny = 10.0 ** rs.uniform(-300, 0, size=(T, G))
    tiny[rs.rand(T, G) < 0.2] = 0.0
    tiny[0, :min(G, 3)] = (1e-300, 0.0, 1.0)[:min(G, 3)]
    exact = rs.randint(0, 2 ** 40, size=(T, G)).astype(np.float64) * 2.0 ** -30
    return {'tiny': tiny, 'exact': exact}
