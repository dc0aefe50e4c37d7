// test_verify_pow.cpp — the grinding nonce in stark101::verify_fri_batch and
// verify_fibsq_batch of the C++ host mirror (stark-prover_amd/host/stark101.hpp,
// fri_verify_batch_pow): transcripts that carry an 8-byte nonce after the final
// value, checked in one device call with the decision of verify_fri /
// verify_fibsq at the same grinding_bits.
//
// Group `cpu` (no device): the empty batch and grinding_bits above 32, and the
// packer's decisions about the nonce message (missing, 4 bytes, doubled, a
// ground transcript packed without bits).
// Group `gpu`: 4 members at (log_t 3, blowup 4) with 2 queries from
// prove_fibsq_batch at 8 bits, all accepted; a flipped nonce byte in member 2
// rejected for its zero bits or its channel; no bits, all rejected; the result
// equals a loop of verify_fibsq.
//
//   test_verify_pow [cpu|gpu|all]
#include <cstdio>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "stark101.hpp"

using namespace stark101;
using Msgs = std::vector<std::vector<uint8_t>>;

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

template <class F>
static bool panics(F&& f) {
    try {
        f();
    } catch (const Panic&) {
        return true;
    }
    return false;
}

// ---------------------------------------------------------------- cpu group
TEST(cpu, empty_batch_and_bits_above_32) {
    const FE g(FRI_GENERATOR);
    ASSERT_TRUE(verify_fri_batch({}, 6, {}, 2, 63, g, {}, nullptr, nullptr, 8).empty());     // no device touched
    ASSERT_TRUE(verify_fibsq_batch({}, {}, 4, 2, 2, {}, g, {}, nullptr, nullptr, 32).empty());
    ASSERT_TRUE(panics([&] { verify_fri_batch({}, 6, {}, 2, 63, g, {}, nullptr, nullptr, 33); }));
    ASSERT_TRUE(panics([&] { verify_fibsq_batch({}, {}, 4, 2, 2, {}, g, {}, nullptr, nullptr, 33); }));
    ASSERT_TRUE(panics([&] { verify_fri({}, 6, 1, 2, 63, g, "", 33); }));                     // as the single verifier
}

// A transcript of the right form for log_n 2, one layer, one query, with a
// nonce (root, final, nonce, index, value, path, sibling value, path); its
// contents are arbitrary: the packer's host decisions depend on the form alone.
static Msgs formed() {
    const std::vector<uint8_t> root(64, 'a'), v = FriChannel::be64(7), path(64, 0x5a);
    return {root, v, FriChannel::be64(0x100000005ull), FriChannel::be64(1), v, path, v, path};
}

TEST(cpu, packer_nonce_rejections) {
    const Msgs ok = formed();
    Msgs missing = ok, four = ok, doubled = ok;
    missing.erase(missing.begin() + 2);
    four[2].resize(4);
    doubled.insert(doubled.begin() + 2, ok[2]);
    const std::vector<Msgs> batch = {missing, four, doubled};
    std::vector<uint32_t> reasons;
    const auto got = verify_fri_batch(batch, 2, {1, 1, 1}, 1, 3, FE(FRI_GENERATOR), {}, nullptr, &reasons, 8);
    ASSERT_TRUE(got.size() == 3 && reasons.size() == 3);
    for (size_t b = 0; b < 3; b++) {
        ASSERT_TRUE(!got[b] && reasons[b] == FRI_VERIFY_MALFORMED);
        ASSERT_TRUE(!verify_fri(batch[b], 2, 1, 1, 3, FE(FRI_GENERATOR), "", 8));
    }
    // a transcript with a nonce, packed without bits: one message too many
    reasons.clear();
    ASSERT_TRUE(!verify_fri_batch({ok}, 2, {1}, 1, 3, FE(FRI_GENERATOR), {}, nullptr, &reasons)[0]);
    ASSERT_TRUE(reasons.size() == 1 && reasons[0] == FRI_VERIFY_MALFORMED && !verify_fri(ok, 2, 1, 1, 3));
    static_assert(FRI_VERIFY_POW == 128u, "fri_amd.h");
}

// ---------------------------------------------------------------- gpu group
TEST(gpu, ground_batch_equals_a_loop_of_verify_fibsq) {
    const uint32_t log_t = 3, lb = 2, bits = 8;
    const size_t q = 2;
    const FE g(FRI_GENERATOR);
    auto gpu = std::make_shared<Gpu>(0, 12);
    const std::vector<FE> a1 = {FE(3141592), FE(7), FE(FRI_P - 2), FE(12345)};
    for (const bool device_queries : {false, true}) {
        std::vector<FriChannel> ch(4);
        const std::vector<uint8_t> hello = {'h', 'i'};
        ch[3].send(hello);                                              // member 3's channel does not start empty
        const std::string state3 = ch[3].state;
        const auto proofs = prove_fibsq_batch(a1, log_t, lb, q, ch, g, gpu, device_queries, bits);
        std::vector<Msgs> t;
        std::vector<FE> a_last;
        std::vector<size_t> nl;
        for (size_t b = 0; b < 4; b++) {
            t.emplace_back(ch[b].proof.begin() + (b == 3 ? 1 : 0), ch[b].proof.end());
            a_last.push_back(proofs[b].a_last);
            nl.push_back(proofs[b].fri.n_layers());
        }
        const std::vector<std::string> states = {"", "", "", state3};
        std::vector<uint32_t> reasons;
        auto got = verify_fibsq_batch(t, a_last, log_t, lb, q, nl, g, states, gpu, &reasons, bits);
        for (size_t b = 0; b < 4; b++) {
            ASSERT_TRUE(verify_fibsq(t[b], a_last[b], log_t, lb, q, nl[b], g, states[b], bits));
            ASSERT_TRUE(got[b] && reasons[b] == 0);
        }
        // without bits the nonce stands where an index is expected
        got = verify_fibsq_batch(t, a_last, log_t, lb, q, nl, g, states, gpu, &reasons);
        for (size_t b = 0; b < 4; b++)
            ASSERT_TRUE(!got[b] && reasons[b] != 0 && !verify_fibsq(t[b], a_last[b], log_t, lb, q, nl[b], g, states[b]));
        // one flipped nonce byte in member 2: trace root, 3 alphas, per layer (root, beta), the final value, the nonce
        const size_t pos = 4 + 2 * nl[2];
        ASSERT_TRUE(t[2][pos].size() == 8);
        t[2][pos][7] ^= 1;
        got = verify_fibsq_batch(t, a_last, log_t, lb, q, nl, g, states, gpu, &reasons, bits);
        for (size_t b = 0; b < 4; b++) {
            ASSERT_TRUE(got[b] == verify_fibsq(t[b], a_last[b], log_t, lb, q, nl[b], g, states[b], bits));
            ASSERT_TRUE(got[b] == (b != 2) && (reasons[b] != 0) == (b == 2));
        }
        ASSERT_TRUE(reasons[2] & (FRI_VERIFY_POW | FRI_VERIFY_CHANNEL));
        ASSERT_TRUE(!(reasons[2] & ~uint32_t{FRI_VERIFY_POW | FRI_VERIFY_CHANNEL}));          // the openings are claimed ones
    }
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
