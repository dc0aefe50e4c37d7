// Times the C++ host mirror's verifiers on transcripts of prove_fibsq_batch
// (tools/batch_probe.py --verify runs it): the baselines of the batched
// verifier and the mirror's whole call.
//   make -C stark-prover_amd verify_native
//   build/verify_native [log_t=7] [log_blowup=3] [queries=8] [batch=256] [reps=5] [threads=16] [grinding_bits=0]
// Proves (and verifies) with `grinding_bits` bits of proof of work.
// Proves min(batch, 256) members once and repeats them up to `batch`, then
// prints one JSON object with the medians, in microseconds per proof:
//   loop_1      a loop of verify_fibsq on one core (over min(batch, 256) members)
//   loop_n      the same loop split over `threads` threads
//   batch_whole verify_fibsq_batch: packing in the mirror and the device call
// Exit status 0 only if every verifier accepts every member.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>

#include "stark101.hpp"

using namespace stark101;
using Msgs = std::vector<std::vector<uint8_t>>;

template <class F>
static double median_us(F&& f, int reps, size_t per) {
    std::vector<double> t;
    for (int i = 0; i < reps; i++) {
        const auto t0 = std::chrono::steady_clock::now();
        f();
        t.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / per);
    }
    std::sort(t.begin(), t.end());
    return t[t.size() / 2];
}

int main(int argc, char** argv) {
    const uint32_t log_t = argc > 1 ? static_cast<uint32_t>(std::atoi(argv[1])) : 7;
    const uint32_t lb = argc > 2 ? static_cast<uint32_t>(std::atoi(argv[2])) : 3;
    const size_t q = argc > 3 ? static_cast<size_t>(std::atoi(argv[3])) : 8;
    const size_t B = argc > 4 ? static_cast<size_t>(std::atoi(argv[4])) : 256;
    const int reps = argc > 5 ? std::atoi(argv[5]) : 5;
    const unsigned threads = argc > 6 ? static_cast<unsigned>(std::atoi(argv[6])) : 16;
    const uint32_t bits = argc > 7 ? static_cast<uint32_t>(std::atoi(argv[7])) : 0;
    try {
        auto gpu = std::make_shared<Gpu>(0, std::max<uint32_t>(12, log_t + lb));
        const size_t m = std::min<size_t>(B, 256);
        std::vector<FE> a1;
        for (size_t b = 0; b < m; b++) a1.push_back(FE(1000003 * b + 3141592));
        std::vector<FriChannel> ch(m);
        const auto proofs = prove_fibsq_batch(a1, log_t, lb, q, ch, FE(FRI_GENERATOR), gpu, false, bits);
        std::vector<Msgs> t;
        std::vector<FE> a_last;
        std::vector<size_t> nl;
        for (size_t b = 0; b < B; b++) {
            t.push_back(ch[b % m].proof);
            a_last.push_back(proofs[b % m].a_last);
            nl.push_back(proofs[b % m].fri.n_layers());
        }
        std::atomic<size_t> accepted{0};
        auto loop = [&](size_t lo, size_t hi) {
            size_t ok = 0;
            for (size_t b = lo; b < hi; b++) ok += verify_fibsq(t[b], a_last[b], log_t, lb, q, nl[b], FE(FRI_GENERATOR), "", bits);
            accepted += ok;
        };
        const double loop_1 = median_us([&] { loop(0, m); }, reps, m);
        const double loop_n = median_us(
            [&] {
                std::vector<std::thread> th;
                for (unsigned i = 0; i < threads; i++) th.emplace_back(loop, m * i / threads, m * (i + 1) / threads);
                for (auto& x : th) x.join();
            },
            reps, m);
        bool ok = accepted == 2 * static_cast<size_t>(reps) * m;
        std::vector<bool> got = verify_fibsq_batch(t, a_last, log_t, lb, q, nl, FE(FRI_GENERATOR), {}, gpu, nullptr, bits);   // warm
        const double whole = median_us(
            [&] { got = verify_fibsq_batch(t, a_last, log_t, lb, q, nl, FE(FRI_GENERATOR), {}, gpu, nullptr, bits); }, reps, B);
        for (bool g : got) ok = ok && g;
        std::printf("{\"loop_1\": %.2f, \"loop_n\": %.2f, \"batch_whole\": %.2f, \"threads\": %u, \"batch\": %zu, "
                    "\"accepted\": %s}\n",
                    loop_1, loop_n, whole, threads, B, ok ? "true" : "false");
        return ok ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("{\"error\": \"%s\"}\n", e.what());
        return 2;
    }
}
