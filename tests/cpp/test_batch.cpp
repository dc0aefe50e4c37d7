// test_batch.cpp — stark101::fri_commit_batch of the C++ host mirror
// (stark-prover_amd/host/stark101.hpp; fri_commit.rs:72-122 for every member,
// in one device call).
//
// Group `cpu` (no device): the constants of the C ABI, the empty batch.
// Group `gpu`: 4 polynomials (one shorter: padded) at 2^10 through
// fri_commit_batch; each channel's messages equal those of fri_commit_coset
// run one by one; decommit_fri on member 2 verifies, in both of its forms;
// a later commit on the Gpu ends the members' residency.
//
//   test_batch [cpu|gpu|all]
#include <cstdio>
#include <functional>
#include <memory>
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
TEST(cpu, constants_and_the_empty_batch) {
    ASSERT_TRUE(FRI_BATCH_MAX_LOG_N >= 14 && FRI_BATCH_MAX_LOG_N <= 18);
    ASSERT_TRUE(FRI_BATCH_LDE_LDS_MAX_LOG_N < FRI_BATCH_MAX_LOG_N);
    std::vector<FriChannel> none;
    ASSERT_TRUE(fri_commit_batch({}, 10, FE(FRI_GENERATOR), none, nullptr).empty());   // no device touched
    std::printf("constants %d %d\n", (int)FRI_BATCH_MAX_LOG_N, (int)FRI_BATCH_LDE_LDS_MAX_LOG_N);
}

// ---------------------------------------------------------------- gpu group
TEST(gpu, members_equal_single_commits_and_decommit) {
    const uint32_t log_n = 10;
    const size_t n = (size_t)1 << log_n;
    const FE offset(FRI_GENERATOR);
    auto gpu = std::make_shared<Gpu>(0, 12);
    std::vector<Poly> polys;
    for (uint64_t b = 0; b < 4; b++) polys.emplace_back(seeded(4100 + b, b == 1 ? 77 : 128));   // one ragged member
    // one by one (member 3's channel does not start empty)
    std::vector<FriChannel> want(4), got(4);
    const std::vector<uint8_t> hello = {'h', 'i'};
    want[3].send(hello);
    got[3].send(hello);
    for (size_t b = 0; b < 4; b++) fri_commit_coset(polys[b], log_n, offset, want[b], gpu);
    const auto proofs = fri_commit_batch(polys, log_n, offset, got, gpu);
    ASSERT_TRUE(proofs.size() == 4);
    for (size_t b = 0; b < 4; b++) {
        ASSERT_TRUE(proofs[b].member() == (int)b && proofs[b].resident());
        ASSERT_TRUE(got[b].proof == want[b].proof && got[b].state == want[b].state);
        ASSERT_TRUE(got[b].compressed_proof == want[b].compressed_proof);
    }
    // the members' layers are their own
    const auto l0 = proofs[0].fri_layer(0), l2 = proofs[2].fri_layer(0);
    ASSERT_TRUE(l0.size() == n && l2.size() == n && l0 != l2);
    ASSERT_TRUE(l2[5] == polys[2].evaluate(offset * omega(log_n).pow(5)));
    // member 2: decommit, verify, reject a flipped bit
    FriChannel ch = got[2];
    decommit_fri(3, n - 1, proofs[2], ch);
    ASSERT_TRUE(verify_fri(ch.proof, log_n, proofs[2].n_layers(), 3, n - 1, offset));
    auto bad = ch.proof;
    bad[bad.size() / 2][0] ^= 1;
    ASSERT_TRUE(!verify_fri(bad, log_n, proofs[2].n_layers(), 3, n - 1, offset));
    // the reference's own form, through the member's layers and device-backed trees
    FriChannel ch2 = got[2];
    decommit_fri(3, n - 1, proofs[2].fri_layers(), proofs[2].fri_merkles, ch2);
    ASSERT_TRUE(ch2.proof == ch.proof && ch2.state == ch.state);
    ASSERT_TRUE(proofs[2].fri_merkles[1].get_authentication_path(7).size() == 32 * (log_n - 1));
    // one by one again on the same Gpu: the single path survived, the members' residency ended
    FriChannel again;
    fri_commit_coset(polys[0], log_n, offset, again, gpu);
    ASSERT_TRUE(again.proof == want[0].proof);
    ASSERT_TRUE(!proofs[2].resident());
    bool threw = false;
    try {
        (void)proofs[2].fri_layer(0);
    } catch (const Panic&) {
        threw = true;
    }
    ASSERT_TRUE(threw);
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
