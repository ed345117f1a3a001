// Stand-alone host program around bllp::check_program (bayesloop_amd/csrc/blhip_likprog.hpp), the validation behind
// blhip_host_lik_program_check / blhip_set_lik_program: meant to be built with the host sanitizers and run on a CPU,
//     hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined --offload-arch=gfx950 tests/host/likprog_check_main.cpp -o likprog_check && ./likprog_check
// It feeds the function valid programs, every kind of broken one and 20 000 random ones (all of which it must classify without reading
// outside its arrays: the buffers are sized exactly).  Exit status 0: every expectation held.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../bayesloop_amd/csrc/blhip_likprog.hpp"

using namespace bllp;

static int failures = 0;

static int check(const std::vector<int32_t> &ops, int64_t n_consts, int64_t n_step, int ndim, bool with_err = true) {
    std::vector<char> err(with_err ? 96 : 0);          // (short on purpose: the messages are truncated, never overrun)
    return check_program(ops.empty() ? nullptr : ops.data(), (int64_t)ops.size() / 2, n_consts, n_step, ndim, with_err ? err.data() : nullptr, (int)err.size());
}

static void expect(bool ok, const char *what) {
    if (!ok) { std::printf("FAILED: %s\n", what); ++failures; }
}

int main() {
    expect(check({OP_DATA, 0, OP_PARAM, 0, OP_ADD, 0}, 0, 0, 1) == 0, "x + p0");
    expect(check({OP_DATA, 0, OP_PARAM, 0, OP_ADD, 0}, 0, 0, 1, false) == 0, "x + p0, no message buffer");
    expect(check({OP_DATA, 0, OP_ADD, 0}, 0, 0, 1) != 0, "underflow");
    expect(check({OP_DATA, 0, OP_ADD, 0}, 0, 0, 1, false) != 0, "underflow, no message buffer");
    expect(check({}, 0, 0, 1) != 0, "empty");
    expect(check({OP_CONST, 2}, 2, 0, 1) != 0 && check({OP_CONST, 1}, 2, 0, 1) == 0, "CONST range");
    expect(check({OP_STEP, 1}, 0, 1, 1) != 0 && check({OP_STEP, 0}, 0, 1, 1) == 0, "STEP range");
    expect(check({OP_PARAM, 2}, 0, 0, 2) != 0 && check({OP_PARAM, 3}, 0, 0, 4) == 0, "PARAM range");
    expect(check({OP_AXIS, 1}, 4, 0, 1) != 0 && check({OP_AXIS, (3 << 2) | 1}, 4, 0, 2) == 0 && check({OP_AXIS, (4 << 2) | 1}, 4, 0, 2) != 0, "AXIS range");
    expect(check({OP_DATA, 0, OP_POWI, 65}, 0, 0, 1) != 0 && check({OP_DATA, 0, OP_POWI, -64}, 0, 0, 1) == 0, "POWI range");
    expect(check({OP_DATA, 0, OP_DATA, 0}, 0, 0, 1) != 0, "two values left");
    expect(check({OP_DATA, 0, 99, 0}, 0, 0, 1) != 0 && check({OP_DATA, 0, -1, 0}, 0, 0, 1) != 0, "unknown code");
    expect(check({OP_DATA, 0}, 0, 0, 0) != 0 && check({OP_DATA, 0}, 0, 0, 5) != 0, "ndim range");
    std::vector<int32_t> deep, long_;
    for (int k = 0; k < 17; ++k) { deep.push_back(OP_DATA); deep.push_back(0); }
    for (int k = 0; k < 16; ++k) { deep.push_back(OP_ADD); deep.push_back(0); }
    expect(check(deep, 0, 0, 1) != 0, "depth 17");
    deep.erase(deep.begin(), deep.begin() + 2); deep.resize(deep.size() - 2);
    expect(check(deep, 0, 0, 1) == 0, "depth 16");
    long_ = {OP_DATA, 0};
    for (int k = 0; k < 255; ++k) { long_.push_back(OP_NEG); long_.push_back(0); }
    expect(check(long_, 0, 0, 1) == 0, "256 ops");
    long_.push_back(OP_NEG); long_.push_back(0);
    expect(check(long_, 0, 0, 1) != 0, "257 ops");
    std::mt19937 rng(12345);
    int accepted = 0;
    for (int trial = 0; trial < 20000; ++trial) {
        const int n = 1 + (int)(rng() % 40);
        std::vector<int32_t> ops;
        for (int k = 0; k < n; ++k) { ops.push_back((int32_t)(rng() % 26) - 2); ops.push_back((int32_t)(rng() % 13) - 3); }
        accepted += check(ops, (int64_t)(rng() % 6), (int64_t)(rng() % 4), 1 + (int)(rng() % 4)) == 0;
    }
    std::printf("%d of 20000 random programs accepted, %d expectation(s) failed\n", accepted, failures);
    return failures ? 1 : 0;
}
