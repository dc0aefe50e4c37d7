// test_multipoint.cpp — arbitrary-point interpolate() and evaluate_points()
// of the C++ host mirror (stark-prover_amd/host/stark101.hpp;
// src/polynomial/ops.rs:76-83, 239-241 -> interpolation.rs:121-152) on the
// device's product tree (fri_interpolate_points / fri_evaluate).
//
// Group `cpu` (no device): the crossover constants of the C ABI.
// Group `gpu`: a shuffled coset of 2^18 points (beyond the direct kernels'
// 2^17) gives back the polynomial whose evaluate_on_coset gave the values;
// evaluate_points equals the header's host Horner; a repeated point yields the
// reference's zero basis term.
//
//   test_multipoint [cpu|gpu|all]
#include <algorithm>
#include <cstdio>
#include <functional>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "stark101.hpp"

using namespace stark101;

// ------------------------------------------------------------ tiny harness
struct Failure {
    std::string msg;
};
#define ASSERT_TRUE(c)                                                                               \
    do {                                                                                             \
        if (!(c)) throw Failure{std::string(__FILE__ ":") + std::to_string(__LINE__) + ": " #c};     \
    } while (0)

struct Test {
    const char* group;
    const char* name;
    std::function<void()> fn;
};
static std::vector<Test>& registry() {
    static std::vector<Test> r;
    return r;
}
struct Reg {
    Reg(const char* g, const char* n, std::function<void()> f) { registry().push_back({g, n, std::move(f)}); }
};
#define TEST(group, name)                                   \
    static void group##_##name();                           \
    static Reg reg_##group##_##name(#group, #name, group##_##name); \
    static void group##_##name()

static std::vector<FE> seeded(uint64_t seed, size_t n) {
    std::vector<FE> c(n);
    uint64_t x = seed;
    for (size_t i = 0; i < n; i++) {
        x += 0x9E3779B97F4A7C15ull;
        uint64_t z = x;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        c[i] = FE(z ^ (z >> 31));
    }
    return c;
}

// ---------------------------------------------------------------- cpu group
TEST(cpu, crossovers_are_powers_of_two) {
    ASSERT_TRUE(FRI_MP_EVAL_MIN > 0 && (FRI_MP_EVAL_MIN & (FRI_MP_EVAL_MIN - 1)) == 0);
    ASSERT_TRUE(FRI_MP_INTERP_MIN > 0 && (FRI_MP_INTERP_MIN & (FRI_MP_INTERP_MIN - 1)) == 0);
    ASSERT_TRUE(FRI_MP_INTERP_MIN <= (1u << 17));                  // the direct kernels' limit
    ASSERT_TRUE((FRI_MP_FORCE_TREE | FRI_MP_FORCE_DIRECT | FRI_MP_SMALL_LEAF) == 7u);
    std::printf("constants %u %u\n", (unsigned)FRI_MP_EVAL_MIN, (unsigned)FRI_MP_INTERP_MIN);
}

// ---------------------------------------------------------------- gpu group
TEST(gpu, interpolate_shuffled_coset_beyond_the_direct_limit) {
    const uint32_t log_n = 18;
    const size_t n = (size_t)1 << log_n;
    auto c = seeded(1801, n);
    c[n - 1] = FE(0);                                              // the interpolant trims
    const Poly f(c);
    const Coset coset(FE(FRI_GENERATOR), omega(log_n), n);
    const auto dom = coset.generate_coset_domain();
    const auto vals = evaluate_on_coset(f, coset);
    std::vector<size_t> perm(n);
    std::iota(perm.begin(), perm.end(), (size_t)0);
    std::shuffle(perm.begin(), perm.end(), std::mt19937_64(18));
    std::vector<FE> xs(n), ys(n);
    for (size_t i = 0; i < n; i++) xs[i] = dom[perm[i]], ys[i] = vals[perm[i]];
    const Poly g = interpolate(xs, ys);
    ASSERT_TRUE(g.coefficients == f.coefficients && g.degree == f.degree);
}
TEST(gpu, evaluate_points_equals_host_horner) {
    const Poly f(seeded(1802, 3000));
    auto xs = seeded(1803, 5000);
    xs[0] = FE(0), xs[1] = FE(1), xs[2] = FE(P - 1), xs[4999] = xs[17];
    const auto got = evaluate_points(f, xs);
    ASSERT_TRUE(got.size() == xs.size());
    for (size_t i = 0; i < xs.size(); i++) ASSERT_TRUE(got[i] == f.evaluate(xs[i]));
    ASSERT_TRUE(evaluate_points(f, std::vector<FE>{}).empty());
    ASSERT_TRUE(evaluate_points(Poly(), xs) == std::vector<FE>(xs.size()));
}
TEST(gpu, evaluate_points_on_the_tree) {
    // min(len, count) = FRI_MP_EVAL_MIN: the automatic choice takes the tree
    const size_t n = FRI_MP_EVAL_MIN;
    const Poly f(seeded(1804, n));
    const auto xs = seeded(1805, n);
    const auto got = evaluate_points(f, xs);
    for (size_t i = 0; i < n; i += 257) ASSERT_TRUE(got[i] == f.evaluate(xs[i]));
    ASSERT_TRUE(got[n - 1] == f.evaluate(xs[n - 1]));
}
TEST(gpu, interpolate_repeated_point_gives_zero_terms) {
    // (1, 5), (2, 7), (2, 9), (4, 3): both copies of x = 2 drop out (inverse(0) = 0,
    // element.rs:54-57), leaving y_0 L_0 + y_3 L_3 over all four points
    const std::vector<FE> xs = {FE(1), FE(2), FE(2), FE(4)}, ys = {FE(5), FE(7), FE(9), FE(3)};
    const Poly g = interpolate(xs, ys);
    Poly want;
    for (size_t i : {size_t(0), size_t(3)}) {
        Poly num(std::vector<FE>{FE(1)});
        FE den = FE::one();
        for (size_t j = 0; j < 4; j++) {
            if (j == i) continue;
            num = num * Poly(std::vector<FE>{FE(0) - xs[j], FE(1)});
            den = den * (xs[i] - xs[j]);
        }
        want = want + num * Poly(std::vector<FE>{ys[i] * den.inverse()});
    }
    ASSERT_TRUE(g == want);
    ASSERT_TRUE(g.evaluate(FE(1)) == FE(5) && g.evaluate(FE(4)) == FE(3) && g.evaluate(FE(2)) == FE::zero());
}

int main(int argc, char** argv) {
    const std::string which = argc > 1 ? argv[1] : "cpu";
    int fails = 0, ran = 0;
    for (auto& t : registry()) {
        if (which != "all" && which != t.group) continue;
        ran++;
        try {
            t.fn();
            std::printf("ok   %s::%s\n", t.group, t.name);
        } catch (const Failure& f) {
            fails++;
            std::printf("FAIL %s::%s: %s\n", t.group, t.name, f.msg.c_str());
        } catch (const std::exception& e) {
            fails++;
            std::printf("FAIL %s::%s: exception: %s\n", t.group, t.name, e.what());
        }
    }
    std::printf("%d tests, %d failures\n", ran, fails);
    return fails;
}
