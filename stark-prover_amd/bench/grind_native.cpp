// Times the C++ host mirror's grinding loop (stark101::grind_host), the
// baseline of tools/grind_probe.py.  Needs no device.
//   make -C stark-prover_amd grind_native
//   build/grind_native [log_count=22] [reps=5] [threads=16] [bits...]
// Every thread walks its own range of 2^log_count nonces at 32 bits behind
// its own state (a range that holds a hit ends the walk early and is counted
// by what it walked).  Prints one JSON object:
//   rate_1      nonces per second of one core (median of reps)
//   rate_n      ... of `threads` threads together
//   grind_us    for each of the given `bits`, the median microseconds of one
//               whole grind_host from nonce 0 over 32 distinct states
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "stark101.hpp"

using namespace stark101;

static double seconds(const std::chrono::steady_clock::time_point& t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
static std::string state_of(unsigned i) { return sha::digest_hex("grind native " + std::to_string(i)); }
static double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

// nonces walked per second by `threads` threads, each over its own 2^log_count
static double rate(unsigned threads, uint32_t log_count) {
    std::vector<uint64_t> walked(threads, 0);
    const uint64_t count = uint64_t{1} << log_count;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> th;
    for (unsigned w = 0; w < threads; w++)
        th.emplace_back([&, w] {
            uint64_t nonce = 0;
            const bool found = grind_host(state_of(w), 32, 0, count - 1, &nonce);
            walked[w] = found ? nonce + 1 : count;
        });
    for (auto& t : th) t.join();
    const double s = seconds(t0);
    uint64_t total = 0;
    for (uint64_t w : walked) total += w;
    return static_cast<double>(total) / s;
}

int main(int argc, char** argv) {
    const uint32_t log_count = argc > 1 ? static_cast<uint32_t>(std::atoi(argv[1])) : 22;
    const int reps = argc > 2 ? std::atoi(argv[2]) : 5;
    const unsigned threads = argc > 3 ? static_cast<unsigned>(std::atoi(argv[3])) : 16;
    std::vector<double> r1, rn;
    for (int i = 0; i < reps; i++) {
        r1.push_back(rate(1, log_count));
        rn.push_back(rate(threads, log_count));
    }
    std::printf("{\"log_count\": %u, \"threads\": %u, \"sha_accelerated\": %s, \"rate_1\": %.0f, \"rate_n\": %.0f, "
                "\"grind_us\": {",
                log_count, threads, sha::accelerated() ? "true" : "false", median(r1), median(rn));
    for (int a = 4; a < argc; a++) {
        const uint32_t bits = static_cast<uint32_t>(std::atoi(argv[a]));
        std::vector<double> us;
        for (unsigned i = 0; i < 32; i++) {
            uint64_t nonce = 0;
            const std::string st = state_of(1000 + i);
            const auto t0 = std::chrono::steady_clock::now();
            grind_host(st, bits, 0, ~uint64_t{0}, &nonce);
            us.push_back(seconds(t0) * 1e6);
        }
        std::printf("%s\"%u\": %.2f", a > 4 ? ", " : "", bits, median(us));
    }
    std::printf("}}\n");
    return 0;
}
