// Tap tables of the transition models' kernels: SciPy's gaussian_filter1d weights, spline shifts, alpha-stable and bivariate kernels
// (reference: transitionModels.py:96-118, :196-260, :571-602, :898-911).  Host only; needs BIGSHIFT_LW2 (blhip_kernels.hpp) in front of it.
// In the library it is included by blhip_program.hpp, INSIDE the anonymous namespace of blhip.hip.
#pragma once

struct TapTable {
    std::vector<double> w;       // concatenated half kernels: w[off + k], k = 0..lw
    std::vector<int> off, lw, lw2;   // lw2: axis-1 radius of a dense 2-D kernel (0 for 1-D tap sets)
    std::map<std::pair<int, double>, int> index;   // (internal axis, normed sigma) -> id
    std::map<std::tuple<double, double, double>, int> index2;   // dense kernels: (ns1, ns2, rho) -> id

    // Deterministic (transitionModels.py:581, :600): scipy.ndimage.shift(order=3, mode='nearest') by d grid cells = stencil
    // out[i] = sum_m K[m] ext[i + m], K[m] = eta(-d - m) with the cardinal cubic spline eta(u) = sum_n sqrt(3) pole^|n| beta3(u - n)
    // (prefilter impulse response x B-spline), |m| <= ceil|d| + 34, over the extension blk::extend_index(rule 2) builds.
    // Exact for |d| <= 12 (beyond, SciPy extends the COEFFICIENTS by their edge values: oracle/bl_oracle.py).  Stored with all
    // 2 lw + 1 weights; lw2 = -1 marks the asymmetric layout.
    struct PairHash { size_t operator()(const std::pair<int, double> &k) const { unsigned long long b; std::memcpy(&b, &k.second, 8); return (size_t)((b * 0x9E3779B97F4A7C15ull) >> 7) ^ (size_t)k.first; } };
    struct DblHash { size_t operator()(double d) const { unsigned long long b; std::memcpy(&b, &d, 8); return (size_t)((b * 0x9E3779B97F4A7C15ull) >> 7); } };
    std::unordered_map<std::pair<int, double>, int, PairHash> index_shift;      // (looked up once per step and chain inside a Deterministic segment)
    int get_shift(int axis, double d) {
        auto key = std::make_pair(axis, d);
        auto it = index_shift.find(key);
        if (it != index_shift.end()) return it->second;
        const double pole = std::sqrt(3.0) - 2.0, gain = -6.0 * pole / (1.0 - pole * pole);
        const int r = (int)std::ceil(std::fabs(d)) + 34;
        const int id = (int)off.size();
        off.push_back((int)w.size());
        lw.push_back(r);
        lw2.push_back(-1);
        for (int m = -r; m <= r; ++m) {
            const double u = -d - (double)m, n0 = std::floor(u);
            double eta = 0.0;
            for (int k = -1; k <= 2; ++k) {
                const double n = n0 + k, a = std::fabs(u - n);
                const double b3 = a < 1.0 ? 2.0 / 3.0 - a * a + a * a * a / 2.0 : (a < 2.0 ? (2.0 - a) * (2.0 - a) * (2.0 - a) / 6.0 : 0.0);
                eta += gain * std::pow(pole, std::fabs(n)) * b3;
            }
            w.push_back(eta);
        }
        index_shift[key] = id;
        return id;
    }

    // The same shift for |d| > 12 grid cells per step (1-D grids; the reference's published break-point study shifts by up to 334 cells
    // per step: docs/source/tutorials/changepointstudy.ipynb).  Beyond its 12 pre-padded samples SciPy extends the spline COEFFICIENTS by
    // their edge values, which no shift-invariant stencil reproduces: the step kernel then works in the two stages of
    // oracle/bl_oracle.py: spline_shift_nearest -- prefilter the padded row (symmetric, radius 34, weights below), then evaluate the cubic
    // B-spline at the shifted coordinates with the coefficient index clamped.  Stored as [d, g(0) .. g(34)]; lw = 12 + 34 is the halo the
    // row needs, lw2 = -2 marks the layout.
    std::unordered_map<double, int, DblHash> index_bigshift;
    int get_bigshift(double d) {
        auto it = index_bigshift.find(d);
        if (it != index_bigshift.end()) return it->second;
        const double pole = std::sqrt(3.0) - 2.0, gain = -6.0 * pole / (1.0 - pole * pole);
        const int id = (int)off.size();
        off.push_back((int)w.size());
        lw.push_back(12 + 34);
        lw2.push_back(-2);
        w.push_back(d);
        for (int m = 0; m <= 34; ++m) w.push_back(gain * std::pow(pole, (double)m));
        index_bigshift[d] = id;
        return id;
    }

    // ... and on grids with two parameters: a stage of its own, run by blk::bigshift_kernel (blhip_bigshift.hpp), which prefilters whole lines
    // by SciPy's recursion and needs the shift alone.  Stored as [d]; lw = 0 (no halo: the tile geometry of the other kernels does not see
    // it), lw2 = BIGSHIFT_LW2 marks the layout.
    std::unordered_map<double, int, DblHash> index_bigshift2;
    int get_bigshift2(double d) {
        auto it = index_bigshift2.find(d);
        if (it != index_bigshift2.end()) return it->second;
        const int id = (int)off.size();
        off.push_back((int)w.size());
        lw.push_back(0);
        lw2.push_back(BIGSHIFT_LW2);
        w.push_back(d);
        index_bigshift2[d] = id;
        return id;
    }

    // AlphaStableRandomWalk.createKernel (transitionModels.py:196-240) for an axis of n points: k[d], d = 0 .. n-1, of the
    // inverse real DFT (numpy.fft.irfft) of exp(-|c w|^alpha) sampled at m = int(3n/2 + 1) points of [0, pi]; the reference's
    // roll + 3x zero padding + fftconvolve(mode='same') (:233-260) is out[i] = sum_j in[j] k[|i - j|] inside the grid
    std::map<std::tuple<int, double, double, int>, int> index_as;
    int get_alphastable(int axis, double c, double alpha, int n) {
        auto key = std::make_tuple(axis, c, alpha, n);
        auto it = index_as.find(key);
        if (it != index_as.end()) return it->second;
        const int m = (int)(3.0 * n / 2.0 + 1.0), K = 2 * (m - 1);
        std::vector<double> X(m);
        for (int q = 0; q < m; ++q) X[q] = std::exp(-std::pow(std::fabs(c * (M_PI * q / (m - 1))), alpha));
        const int id = (int)off.size();
        off.push_back((int)w.size());
        lw.push_back(n - 1);
        lw2.push_back(0);
        for (int j = 0; j < n; ++j) {
            long double acc = X[0] + ((j & 1) ? -X[m - 1] : X[m - 1]);
            for (int q = 1; q < m - 1; ++q)
                acc += 2.0L * X[q] * std::cos(2.0L * (long double)M_PIl * (long double)(((long long)j * q) % K) / (long double)K);
            w.push_back((double)(acc / K));
        }
        index_as[key] = id;
        return id;
    }

    // BivariateRandomWalk.createKernel (transitionModels.py:898-911): bivariate normal density on the integer lattice
    // |x| <= 3 ceil(ns1), |y| <= 3 ceil(ns2), normalised to sum 1 (the density's own constant cancels); row-major
    int get2d(double ns1, double ns2, double rho) {
        auto key = std::make_tuple(ns1, ns2, rho);
        auto it = index2.find(key);
        if (it != index2.end()) return it->second;
        const int r0 = 3 * (int)std::ceil(ns1), r1 = 3 * (int)std::ceil(ns2);
        std::vector<double> k((size_t)(2 * r0 + 1) * (2 * r1 + 1));
        double sum = 0.0;
        for (int a = -r0; a <= r0; ++a)
            for (int b = -r1; b <= r1; ++b) {
                const double x = a, y = b;
                const double q = (x * x / (ns1 * ns1) - 2.0 * rho * x * y / (ns1 * ns2) + y * y / (ns2 * ns2)) / (2.0 * (1.0 - rho * rho));
                const double v = std::exp(-q);
                k[(size_t)(a + r0) * (2 * r1 + 1) + (b + r1)] = v;
                sum += v;
            }
        const int id = (int)off.size();
        off.push_back((int)w.size());
        lw.push_back(r0);
        lw2.push_back(r1);
        for (double v : k) w.push_back(v / sum);
        index2[key] = id;
        return id;
    }

    // SciPy's kernel: lw = int(4 sd + 0.5); phi = exp(-0.5/sd^2 x^2); phi / sum(phi)   (_filters.py, gaussian_filter1d)
    int get(int axis, double ns) {
        auto key = std::make_pair(axis, ns);
        auto it = index.find(key);
        if (it != index.end()) return it->second;
        const int r = (int)(4.0 * ns + 0.5);
        int id = -1;
        if (r > 0) {
            std::vector<double> phi(2 * r + 1);
            const double s2 = ns * ns;
            double sum = 0.0;
            for (int k = -r; k <= r; ++k) {
                phi[k + r] = std::exp(-0.5 / s2 * (double)(k * k));
                sum += phi[k + r];
            }
            id = (int)off.size();
            off.push_back((int)w.size());
            lw.push_back(r);
            lw2.push_back(0);
            for (int k = 0; k <= r; ++k) w.push_back(phi[r + k] / sum);
        }
        index[key] = id;
        return id;
    }
};
