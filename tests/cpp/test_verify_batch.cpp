// test_verify_batch.cpp — stark101::verify_fri_batch and verify_fibsq_batch of
// the C++ host mirror (stark-prover_amd/host/stark101.hpp): many transcripts of
// one shape checked in one device call, with the decision of verify_fri /
// verify_fibsq for every one.
//
// Group `cpu` (no device): the empty batch, size mismatches, and the members
// the packer decides on the host (a short and a long transcript, a value >= p,
// a root that is not lowercase hex).
// Group `gpu`: 4 members at (log_t 8, blowup 8) with 2 queries from
// prove_fibsq_batch, all accepted; a flipped byte in member 2 rejected; the
// result equals a loop of verify_fibsq; a plain fri_commit_batch with
// decommit_fri_batch goes through verify_fri_batch.
//
//   test_verify_batch [cpu|gpu|all]
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
TEST(cpu, empty_batch_and_size_mismatch) {
    ASSERT_TRUE(verify_fri_batch({}, 6, {}, 2, 63).empty());            // no device touched
    ASSERT_TRUE(verify_fibsq_batch({}, {}, 4, 2, 2, {}).empty());
    const std::vector<Msgs> one(1);
    ASSERT_TRUE(panics([&] { verify_fri_batch(one, 6, {}, 2, 63); }));
    ASSERT_TRUE(panics([&] { verify_fri_batch(one, 6, {1, 1}, 2, 63); }));
    ASSERT_TRUE(panics([&] { verify_fri_batch(one, 6, {1}, 2, 63, FE(FRI_GENERATOR), {"", ""}); }));
    ASSERT_TRUE(panics([&] { verify_fibsq_batch(one, {}, 4, 2, 2, {1}); }));
    ASSERT_TRUE(panics([&] { verify_fibsq_batch(one, {FE(1)}, 4, 2, 2, {1, 2}); }));
}

// A transcript of the right form for log_n 2, one layer, one query (root,
// final, index, value, path, sibling value, path); its contents are arbitrary:
// the packer's host decisions depend on the form alone.
static Msgs formed() {
    const std::vector<uint8_t> root(64, 'a'), v = FriChannel::be64(7), path(64, 0x5a);
    return {root, v, FriChannel::be64(1), v, path, v, path};
}

TEST(cpu, packer_host_rejections) {
    const Msgs ok = formed();
    Msgs shorter(ok.begin(), ok.end() - 1), longer = ok, big = ok, upper = ok, odd_len = ok;
    longer.push_back(ok.back());
    big[3] = FriChannel::be64(FRI_P);                                   // a value >= p
    upper[0] = std::vector<uint8_t>(64, 'A');                           // not canonical lowercase hex
    odd_len[4].pop_back();                                              // a path of 63 bytes
    const std::vector<Msgs> batch = {shorter, longer, big, upper, odd_len};
    std::vector<uint32_t> reasons;
    const auto got = verify_fri_batch(batch, 2, {1, 1, 1, 1, 1}, 1, 3, FE(FRI_GENERATOR), {}, nullptr, &reasons);
    ASSERT_TRUE(got.size() == 5 && reasons.size() == 5);
    for (size_t b = 0; b < 5; b++) {
        ASSERT_TRUE(!got[b] && reasons[b] == FRI_VERIFY_MALFORMED);
        ASSERT_TRUE(!verify_fri(batch[b], 2, 1, 1, 3));
    }
    // an n_layers out of range is the host verifier's first rejection
    ASSERT_TRUE(!verify_fri_batch({ok}, 2, {4}, 1, 3)[0] && !verify_fri(ok, 2, 4, 1, 3));
    ASSERT_TRUE(!verify_fri_batch({ok}, 2, {0}, 1, 3)[0] && !verify_fri(ok, 2, 0, 1, 3));
}

// ---------------------------------------------------------------- gpu group
TEST(gpu, batch_equals_a_loop_of_verify_fibsq) {
    const uint32_t log_t = 8, lb = 3;
    const size_t q = 2;
    auto gpu = std::make_shared<Gpu>(0, 12);
    const std::vector<FE> a1 = {FE(3141592), FE(7), FE(FRI_P - 2), FE(12345)};
    std::vector<FriChannel> ch(4);
    const std::vector<uint8_t> hello = {'h', 'i'};
    ch[3].send(hello);                                                  // member 3's channel does not start empty
    const std::string state3 = ch[3].state;
    const auto proofs = prove_fibsq_batch(a1, log_t, lb, q, ch, FE(FRI_GENERATOR), gpu);
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
    auto got = verify_fibsq_batch(t, a_last, log_t, lb, q, nl, FE(FRI_GENERATOR), states, gpu, &reasons);
    for (size_t b = 0; b < 4; b++) {
        ASSERT_TRUE(verify_fibsq(t[b], a_last[b], log_t, lb, q, nl[b], FE(FRI_GENERATOR), states[b]));
        ASSERT_TRUE(got[b] && reasons[b] == 0);
    }
    ASSERT_TRUE(proofs[2].fri.resident());                              // the verifier left the batch resident
    // one flipped byte in member 2
    t[2][t[2].size() / 2][0] ^= 1;
    got = verify_fibsq_batch(t, a_last, log_t, lb, q, nl, FE(FRI_GENERATOR), states, gpu, &reasons);
    for (size_t b = 0; b < 4; b++) {
        ASSERT_TRUE(got[b] == verify_fibsq(t[b], a_last[b], log_t, lb, q, nl[b], FE(FRI_GENERATOR), states[b]));
        ASSERT_TRUE(got[b] == (b != 2) && (reasons[b] != 0) == (b == 2));
    }
    // another public output for member 0
    a_last[0] = a_last[0] + FE(1);
    got = verify_fibsq_batch(t, a_last, log_t, lb, q, nl, FE(FRI_GENERATOR), states, gpu);
    ASSERT_TRUE(!got[0] && got[1] && !got[2] && got[3]);
}

TEST(gpu, plain_batch_through_verify_fri_batch) {
    const uint32_t log_n = 10;
    const size_t n = size_t{1} << log_n;
    const FE offset(FRI_GENERATOR);
    auto gpu = std::make_shared<Gpu>(0, 12);
    std::vector<Poly> polys;
    for (uint64_t b = 0; b < 3; b++) {
        std::vector<FE> c(b == 1 ? 1 : 128);                            // member 1 is a constant: one layer
        for (size_t i = 0; i < c.size(); i++) c[i] = FE(1000 * (b + 1) + 7 * i + 1);
        polys.emplace_back(c);
    }
    std::vector<FriChannel> ch(3);
    const auto proofs = fri_commit_batch(polys, log_n, offset, ch, gpu);
    decommit_fri_batch(3, n - 1, proofs, ch);
    std::vector<Msgs> t;
    std::vector<size_t> nl;
    for (size_t b = 0; b < 3; b++) {
        t.push_back(ch[b].proof);
        nl.push_back(proofs[b].n_layers());
        ASSERT_TRUE(verify_fri(t[b], log_n, nl[b], 3, n - 1, offset));
    }
    ASSERT_TRUE(nl[1] == 1 && nl[0] > 1);
    std::vector<uint32_t> reasons;
    auto got = verify_fri_batch(t, log_n, nl, 3, n - 1, offset, {}, gpu, &reasons);
    ASSERT_TRUE(got[0] && got[1] && got[2] && !reasons[0] && !reasons[1] && !reasons[2]);
    t[0].back()[5] ^= 4;                                                // the last sibling path of member 0
    got = verify_fri_batch(t, log_n, nl, 3, n - 1, offset, {}, gpu, &reasons);
    ASSERT_TRUE(!got[0] && got[1] && got[2] && (reasons[0] & FRI_VERIFY_FRI_PATH));
    ASSERT_TRUE(!verify_fri(t[0], log_n, nl[0], 3, n - 1, offset));
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
