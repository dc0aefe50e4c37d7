// test_interpolation.cpp — gen_polynomial_from_roots / gen_lagrange_polynomials
// (_parallel) of the C++ host mirror (stark-prover_amd/host/stark101.hpp;
// src/polynomial/interpolation.rs:9-115).
//
// Group `cpu` (no device): the reference's known answers at modulus 7
// (interpolation.rs:170-221, 259-282, 307-372, the values
// tests/test_oracle_kats.py pins on the oracle) on the header's schoolbook.
// Group `gpu`: the frozen field, whose specialisations run on the device
// (fri_poly_from_roots / fri_lagrange_basis): Z(x_i) = 0, L_i(x_j) = delta_ij.
//
//   test_interpolation [cpu|gpu|all]
#include <cstdio>
#include <functional>
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

using F7 = FieldElement<7>;
static std::vector<F7> v7(std::initializer_list<uint64_t> c) {
    std::vector<F7> v;
    for (uint64_t x : c) v.push_back(F7(x));
    return v;
}

// ---------------------------------------------------------------- cpu group
TEST(cpu, from_roots_known_answer) {                             // interpolation.rs:170-184
    const auto z = gen_polynomial_from_roots<7>(v7({1, 2, 3}));
    ASSERT_TRUE(z.coefficients == v7({1, 4, 1, 1}) && z.degree == 3);
    for (uint64_t r : {1, 2, 3}) ASSERT_TRUE(z.evaluate(F7(r)) == F7::zero());
}
TEST(cpu, empty_input) {
    ASSERT_TRUE(gen_polynomial_from_roots<7>(std::vector<F7>{}).is_zero());
    ASSERT_TRUE(gen_lagrange_polynomials<7>(std::vector<F7>{}).empty());
    ASSERT_TRUE(gen_lagrange_polynomials_parallel<7>(std::vector<F7>{}).empty());
}
TEST(cpu, lagrange_basis_values) {                               // :187-221, :259-282, :307-372
    for (const auto& xs : {v7({2, 3, 5}), v7({2, 3, 5, 6}), v7({1, 2, 3, 4, 6})}) {
        const auto basis = gen_lagrange_polynomials<7>(xs);
        ASSERT_TRUE(basis.size() == xs.size());
        for (size_t i = 0; i < xs.size(); i++) {
            ASSERT_TRUE(basis[i].coefficients.size() == xs.size());
            for (size_t j = 0; j < xs.size(); j++)
                ASSERT_TRUE(basis[i].evaluate(xs[j]) == (i == j ? F7::one() : F7::zero()));
        }
    }
}
TEST(cpu, parallel_equals_serial) {
    for (const auto& xs : {v7({2, 3, 5}), v7({1, 2, 3, 4, 6}), v7({4})}) {
        const auto a = gen_lagrange_polynomials<7>(xs), b = gen_lagrange_polynomials_parallel<7>(xs);
        ASSERT_TRUE(a.size() == b.size());
        for (size_t i = 0; i < a.size(); i++) ASSERT_TRUE(a[i] == b[i] && a[i].degree == b[i].degree);
    }
}
TEST(cpu, repeated_point_gives_zero_rows) {                      // inverse(0) = 0 (element.rs:54-57)
    const auto xs = v7({1, 2, 3, 2, 5});
    const auto basis = gen_lagrange_polynomials<7>(xs);
    for (size_t i : {size_t(1), size_t(3)}) {
        ASSERT_TRUE(basis[i].coefficients == std::vector<F7>(5));   // n zeros, not re-trimmed (ops.rs:194-198)
        ASSERT_TRUE(basis[i].degree == 4);
    }
    ASSERT_TRUE(basis[0].evaluate(F7(1)) == F7::one());
}

// ---------------------------------------------------------------- gpu group
static std::vector<FE> seeded_distinct(uint64_t seed, size_t n) {
    std::vector<FE> c;
    uint64_t x = seed;
    while (c.size() < n) {
        x += 0x9E3779B97F4A7C15ull;
        uint64_t z = x;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        const FE v(z ^ (z >> 31));
        bool seen = false;
        for (const FE& o : c) seen = seen || o == v;
        if (!seen) c.push_back(v);
    }
    return c;
}

TEST(gpu, from_roots_round_trip) {
    const auto xs = seeded_distinct(300, 300);
    const Poly z = gen_polynomial_from_roots<P>(xs);
    ASSERT_TRUE(z.degree == 300 && z.coefficients.back() == FE::one());
    for (const FE& x : xs) ASSERT_TRUE(z.evaluate(x) == FE::zero());
    ASSERT_TRUE(z.evaluate(FE(0)) != FE::zero());
    ASSERT_TRUE(gen_polynomial_from_roots<P>(std::vector<FE>{}).is_zero());
    const Poly lin = gen_polynomial_from_roots<P>(std::vector<FE>{FE(5)});
    ASSERT_TRUE(lin.coefficients == (std::vector<FE>{FE(P - 5), FE(1)}));
}
TEST(gpu, lagrange_round_trip) {
    const auto xs = seeded_distinct(301, 300);
    const auto basis = gen_lagrange_polynomials<P>(xs);
    ASSERT_TRUE(basis.size() == 300);
    for (size_t i = 0; i < 300; i++) {
        ASSERT_TRUE(basis[i].coefficients.size() == 300 && basis[i].degree == 299);
        for (size_t j = 0; j < 300; j++)
            ASSERT_TRUE(basis[i].evaluate(xs[j]) == (i == j ? FE::one() : FE::zero()));
    }
    const auto par = gen_lagrange_polynomials_parallel<P>(xs);
    ASSERT_TRUE(par.size() == 300);
    for (size_t i = 0; i < 300; i++) ASSERT_TRUE(par[i] == basis[i]);
    ASSERT_TRUE(gen_lagrange_polynomials<P>(std::vector<FE>{}).empty());
}
TEST(gpu, lagrange_repeated_point) {
    const std::vector<FE> xs = {FE(1), FE(2), FE(3), FE(2), FE(5)};
    const auto basis = gen_lagrange_polynomials<P>(xs);
    for (size_t i : {size_t(1), size_t(3)}) {
        ASSERT_TRUE(basis[i].coefficients == std::vector<FE>(5) && basis[i].degree == 4);
    }
    ASSERT_TRUE(basis[0].evaluate(FE(1)) == FE::one() && basis[4].evaluate(FE(5)) == FE::one());
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
