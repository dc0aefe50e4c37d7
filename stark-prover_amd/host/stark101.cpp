// stark101.cpp — host side of the C++ mirror (see stark101.hpp).  Everything
// field-sized on the commit path goes through libfri_amd.so; this file holds
// the transcript (SHA-256 on the host, as the reference's Channel does it),
// argument checks that reproduce the reference's panics, and the glue that
// turns fri_commit_result into Channel messages and an FRIProof.
#include "stark101.hpp"

#include <functional>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#if defined(__x86_64__)
#include <cpuid.h>
#include <immintrin.h>
#endif

namespace stark101 {

// ------------------------------------------------------------------ SHA-256
namespace {
constexpr uint32_t K256[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
    0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
    0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
    0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
    0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

inline uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

void compress_scalar(uint32_t h[8], const uint8_t* data, size_t nblocks) {
    for (; nblocks; nblocks--, data += 64) {
        uint32_t w[64];
        for (int i = 0; i < 16; i++)
            w[i] = (uint32_t)data[4 * i] << 24 | (uint32_t)data[4 * i + 1] << 16 | (uint32_t)data[4 * i + 2] << 8 |
                   data[4 * i + 3];
        for (int i = 16; i < 64; i++) {
            uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
            uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
            w[i] = w[i - 16] + s0 + w[i - 7] + s1;
        }
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], k = h[7];
        for (int i = 0; i < 64; i++) {
            uint32_t t1 = k + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K256[i] + w[i];
            uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
            k = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
        h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += k;
    }
}

#if defined(__x86_64__)
// x86 SHA extensions: the transcript hashes ~3000 blocks per STARK-101 proof
// (hex-encoded authentication paths), which dominates the host side of
// prove/verify.  State kept as the instructions want it: ABEF = {F,E,B,A},
// CDGH = {H,G,D,C} (dword 0 first).  Each 4-round group: W+K, two
// sha256rnds2 (rounds 4g, 4g+1 from dwords 0-1, 4g+2, 4g+3 from 2-3); the
// schedule W[t] = s1(W[t-2]) + W[t-7] + s0(W[t-15]) + W[t-16] is msg1 (adds
// s0) + the W[t-7] lane window + msg2 (adds s1 with its in-vector chain).
__attribute__((target("sha,sse4.1,ssse3"))) void compress_shani(uint32_t h[8], const uint8_t* data, size_t nblocks) {
    const __m128i bswap = _mm_set_epi64x(0x0c0d0e0f08090a0bULL, 0x0405060700010203ULL);
    const __m128i abcd = _mm_shuffle_epi32(_mm_loadu_si128(reinterpret_cast<const __m128i*>(h)), 0xB1);      // B,A,D,C
    const __m128i efgh = _mm_shuffle_epi32(_mm_loadu_si128(reinterpret_cast<const __m128i*>(h + 4)), 0x1B);  // H,G,F,E
    __m128i abef = _mm_alignr_epi8(abcd, efgh, 8);     // F,E,B,A
    __m128i cdgh = _mm_blend_epi16(efgh, abcd, 0xF0);  // H,G,D,C
    for (; nblocks; nblocks--, data += 64) {
        const __m128i abef0 = abef, cdgh0 = cdgh;
        __m128i m[4];
        for (int j = 0; j < 4; j++)
            m[j] = _mm_shuffle_epi8(_mm_loadu_si128(reinterpret_cast<const __m128i*>(data + 16 * j)), bswap);
        for (int g = 0; g < 16; g++) {
            if (g >= 4) {
                __m128i x = _mm_sha256msg1_epu32(m[g & 3], m[(g + 1) & 3]);
                x = _mm_add_epi32(x, _mm_alignr_epi8(m[(g + 3) & 3], m[(g + 2) & 3], 4));
                m[g & 3] = _mm_sha256msg2_epu32(x, m[(g + 3) & 3]);
            }
            __m128i wk = _mm_add_epi32(m[g & 3], _mm_loadu_si128(reinterpret_cast<const __m128i*>(K256 + 4 * g)));
            cdgh = _mm_sha256rnds2_epu32(cdgh, abef, wk);            // -> new ABEF; old ABEF is the new CDGH
            wk = _mm_shuffle_epi32(wk, 0x0E);
            abef = _mm_sha256rnds2_epu32(abef, cdgh, wk);
        }
        abef = _mm_add_epi32(abef, abef0);
        cdgh = _mm_add_epi32(cdgh, cdgh0);
    }
    const __m128i feba = _mm_shuffle_epi32(abef, 0x1B);  // A,B,E,F
    const __m128i dchg = _mm_shuffle_epi32(cdgh, 0xB1);  // G,H,C,D
    _mm_storeu_si128(reinterpret_cast<__m128i*>(h), _mm_blend_epi16(feba, dchg, 0xF0));      // A,B,C,D
    _mm_storeu_si128(reinterpret_cast<__m128i*>(h + 4), _mm_alignr_epi8(dchg, feba, 8));     // E,F,G,H
}

bool cpu_has_sha() {
    unsigned a = 0, b = 0, c = 0, d = 0;
    if (!__get_cpuid_count(7, 0, &a, &b, &c, &d)) return false;
    return (b >> 29) & 1u;
}
#endif

void compress_blocks(uint32_t h[8], const uint8_t* data, size_t nblocks) {
#if defined(__x86_64__)
    static const bool ni = cpu_has_sha() && std::getenv("STARK101_NO_SHANI") == nullptr;
    if (ni) {
        compress_shani(h, data, nblocks);
        return;
    }
#endif
    compress_scalar(h, data, nblocks);
}
}  // namespace

namespace sha {
namespace {
std::array<uint8_t, 32> digest_with(void (*fn)(uint32_t*, const uint8_t*, size_t), const uint8_t* data, size_t len) {
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    size_t full = len / 64;
    fn(h, data, full);
    uint8_t tail[128] = {0};
    size_t rem = len - 64 * full;
    if (rem) std::memcpy(tail, data + 64 * full, rem);
    tail[rem] = 0x80;
    size_t tl = rem + 9 <= 64 ? 64 : 128;
    uint64_t bits = static_cast<uint64_t>(len) * 8;
    for (int i = 0; i < 8; i++) tail[tl - 1 - i] = static_cast<uint8_t>(bits >> (8 * i));
    fn(h, tail, tl / 64);
    std::array<uint8_t, 32> out{};
    for (int i = 0; i < 8; i++)
        for (int j = 0; j < 4; j++) out[4 * i + j] = static_cast<uint8_t>(h[i] >> (24 - 8 * j));
    return out;
}
}  // namespace

std::array<uint8_t, 32> digest(const uint8_t* data, size_t len) { return digest_with(compress_blocks, data, len); }
std::array<uint8_t, 32> digest_portable(const uint8_t* data, size_t len) {
    return digest_with(compress_scalar, data, len);
}
bool accelerated() {
#if defined(__x86_64__)
    return cpu_has_sha() && std::getenv("STARK101_NO_SHANI") == nullptr;
#else
    return false;
#endif
}

std::string hex(const uint8_t* data, size_t len) {
    static const char* d = "0123456789abcdef";
    std::string s(2 * len, '0');
    for (size_t i = 0; i < len; i++) {
        s[2 * i] = d[data[i] >> 4];
        s[2 * i + 1] = d[data[i] & 15];
    }
    return s;
}

std::string digest_hex(const std::string& s) {
    auto dg = digest(reinterpret_cast<const uint8_t*>(s.data()), s.size());
    return hex(dg.data(), dg.size());
}

std::vector<uint8_t> from_hex(const std::string& s) {
    if (s.size() % 2) throw Panic("odd-length hex string");
    auto nib = [](char c) -> int {
        if (c >= '0' && c <= '9') return c - '0';
        if (c >= 'a' && c <= 'f') return c - 'a' + 10;
        if (c >= 'A' && c <= 'F') return c - 'A' + 10;
        throw Panic("invalid hex digit");
    };
    std::vector<uint8_t> out(s.size() / 2);
    for (size_t i = 0; i < out.size(); i++) out[i] = static_cast<uint8_t>(nib(s[2 * i]) << 4 | nib(s[2 * i + 1]));
    return out;
}
}  // namespace sha

uint64_t os_random_u64() {
    static thread_local std::random_device rd;      // OsRng (element.rs:32-36)
    return (static_cast<uint64_t>(rd()) << 32) ^ rd();
}

FE omega(uint32_t log_n) {
    if (log_n > 30) throw Panic("no subgroup of order 2^" + std::to_string(log_n));
    return FE(FRI_GENERATOR).pow((P - 1) >> log_n);
}

// ---------------------------------------------------------------------- Gpu
Gpu::Gpu(int device, uint32_t log_n_max) : log_n_max_(log_n_max) {
    int rc = fri_ctx_create(device, log_n_max, &ctx_);
    if (rc != FRI_OK) {
        std::string msg = ctx_ ? fri_last_error(ctx_) : "";
        if (ctx_) fri_ctx_destroy(ctx_);
        ctx_ = nullptr;
        throw Panic("fri_ctx_create failed (code " + std::to_string(rc) + ")" + (msg.empty() ? "" : ": " + msg));
    }
}

Gpu::Gpu(const std::vector<int>& devices, uint32_t log_n_max, int transport)
    : log_n_max_(log_n_max), n_ranks_(static_cast<uint32_t>(devices.size())) {
    int rc = fri_ctx_create_multi(devices.data(), static_cast<uint32_t>(devices.size()), log_n_max, transport, &ctx_);
    if (rc != FRI_OK) {
        ctx_ = nullptr;
        throw Panic("fri_ctx_create_multi failed (code " + std::to_string(rc) + ")");
    }
}

Gpu::Gpu(Default, uint32_t log_n_max) : log_n_max_(log_n_max) {
    int rc = fri_ctx_create_default(log_n_max, &ctx_, &n_ranks_);
    if (rc != FRI_OK) {
        ctx_ = nullptr;
        throw Panic("fri_ctx_create_default failed (code " + std::to_string(rc) +
                    (rc == FRI_EINVAL ? ": malformed FRI_DEVICES / FRI_TRANSPORT)" : ")"));
    }
}

Gpu::~Gpu() {
    if (ctx_) fri_ctx_destroy(ctx_);
}

void Gpu::check(int rc, const char* what) const {
    if (rc != FRI_OK) throw Panic(std::string(what) + ": " + fri_last_error(ctx_) + " (code " + std::to_string(rc) + ")");
}

std::shared_ptr<Gpu> Gpu::thread_default(uint32_t log_n) {
    static thread_local std::shared_ptr<Gpu> g;
    const uint32_t want = log_n < 12 ? 12 : log_n;
    if (!g || g->log_n_max() < want) g = std::make_shared<Gpu>(Gpu::Default{}, want);
    return g;
}

// ------------------------------------------------------------------ grinding
namespace {
uint32_t g_grind_device_min_bits = GRIND_DEVICE_MIN_BITS;

fri_channel_state abi_state(const std::string& state) {
    fri_channel_state c{};
    if (state.empty()) return c;
    if (state.size() != 64) throw Panic("Channel state is not valid hex");
    auto st = sha::from_hex(state);
    std::memcpy(c.digest, st.data(), 32);
    c.has_state = 1;
    return c;
}
void check_grinding_bits(uint32_t bits) {
    if (bits > GRIND_MAX_BITS) throw Panic("grinding_bits must be 0..32");
}
}  // namespace

uint32_t grind_device_min_bits() { return g_grind_device_min_bits; }
void set_grind_device_min_bits(uint32_t bits) { g_grind_device_min_bits = bits; }

bool state_has_zero_bits(const std::string& state, uint32_t bits) {
    if (state.size() != 64 || bits > 256) return false;
    const auto d = sha::from_hex(state);
    for (uint32_t i = 0; i < bits; i++)
        if (d[i / 8] >> (7 - i % 8) & 1) return false;
    return true;
}

bool grind_host(const std::string& state, uint32_t bits, uint64_t first, uint64_t last, uint64_t* nonce) {
    if (bits > GRIND_MAX_BITS || first > last) throw Panic("grind: bits must be 0..32 and first <= last");
    // the state's whole blocks once; then per nonce the tail: the rest of the
    // state, the nonce's 16 hex characters, the padding and the length
    uint32_t mid[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    const size_t full = state.size() / 64, rem = state.size() - 64 * full, len = state.size() + 16;
    compress_blocks(mid, reinterpret_cast<const uint8_t*>(state.data()), full);
    uint8_t tail[128] = {0};
    std::memcpy(tail, state.data() + 64 * full, rem);
    tail[rem + 16] = 0x80;
    const size_t tl = rem + 16 + 9 <= 64 ? 64 : 128;                    // rem < 64
    for (int i = 0; i < 8; i++) tail[tl - 1 - i] = static_cast<uint8_t>(static_cast<uint64_t>(len) * 8 >> (8 * i));
    const uint32_t mask = bits ? ~uint32_t{0} << (32 - bits) : 0;
    static const char* digits = "0123456789abcdef";
    for (uint64_t v = first;; v++) {
        for (int i = 0; i < 16; i++) tail[rem + i] = static_cast<uint8_t>(digits[v >> (60 - 4 * i) & 15]);
        uint32_t h[8];
        std::memcpy(h, mid, sizeof h);
        compress_blocks(h, tail, tl / 64);
        if ((h[0] & mask) == 0) {
            *nonce = v;
            return true;
        }
        if (v == last) return false;
    }
}

bool grind_device(const Gpu& gpu, const std::string& state, uint32_t bits, uint64_t first, uint64_t last,
                  uint64_t* nonce) {
    const fri_channel_state cin = abi_state(state);
    uint32_t found = 0;
    gpu.check(fri_grind(gpu.ctx(), &cin, bits, first, last, nonce, &found, nullptr), "fri_grind");
    return found != 0;
}

namespace {
// A prover's grinding step: nothing for 0 bits, else Channel::grind, on the
// host below grind_device_min_bits() and on the device from it up.
void grind_step(FriChannel& channel, uint32_t bits, const std::shared_ptr<Gpu>& gpu) {
    check_grinding_bits(bits);
    if (bits) channel.grind(bits, bits >= g_grind_device_min_bits ? gpu : nullptr);
}
// ... for every member's channel: on the device ONE fri_grind_batch on the
// members' states; every channel then sends its nonce and must arrive at the
// state the device returned.
void grind_step_batch(std::vector<FriChannel>& channels, uint32_t bits, const Gpu& gpu) {
    check_grinding_bits(bits);
    if (!bits) return;
    if (bits < g_grind_device_min_bits) {
        for (auto& ch : channels) ch.grind(bits);
        return;
    }
    const size_t B = channels.size();
    std::vector<fri_channel_state> chan(B);
    for (size_t b = 0; b < B; b++) chan[b] = abi_state(channels[b].state);
    std::vector<uint64_t> nonces(B);
    std::vector<uint32_t> found(B);
    gpu.check(fri_grind_batch(gpu.ctx(), static_cast<uint32_t>(B), chan.data(), bits, ~uint64_t{0}, nonces.data(),
                              found.data()),
              "fri_grind_batch");
    for (size_t b = 0; b < B; b++) {
        if (!found[b]) throw Panic("grind: member " + std::to_string(b) + ": no nonce gives the state the zero bits");
        channels[b].send(FriChannel::be64(nonces[b]));
        if (channels[b].state != sha::hex(chan[b].digest, 32) || !state_has_zero_bits(channels[b].state, bits))
            throw Panic("grind: member " + std::to_string(b) + ": the state after the nonce is not the device's");
    }
}
}  // namespace

namespace {
uint32_t ceil_log2(size_t n) {
    uint32_t l = 0;
    while ((size_t{1} << l) < n) l++;
    return l;
}

std::vector<uint32_t> to_u32(const std::vector<FE>& v) {
    std::vector<uint32_t> o(v.size());
    for (size_t i = 0; i < v.size(); i++) o[i] = static_cast<uint32_t>(v[i].value());
    return o;
}

std::vector<FE> to_fe(const uint32_t* v, size_t n) {
    std::vector<FE> o(n);
    for (size_t i = 0; i < n; i++) o[i] = FE(v[i]);
    return o;
}

// The device evaluates on offset*<omega_n>: accept exactly that domain.
// Checks the length, D[0] = offset != 0, D[1] = offset*omega_n and the last
// point; the remaining points are the caller's contract (coset_fri.rs:32-36),
// as materialising and comparing 2^24 points would cost more than the commit.
uint32_t coset_log_n(const std::vector<FE>& d, FE* offset) {
    const size_t n = d.size();
    if (n == 0 || (n & (n - 1))) throw Panic("domain size must be a power of two (got " + std::to_string(n) + ")");
    const uint32_t log_n = ceil_log2(n);
    const FE off = d[0], w = omega(log_n);
    if (off == FE::zero()) throw Panic("domain offset must be non-zero");
    if (n > 1 && (d[1] != off * w || d[n - 1] != off * w.pow(n - 1)))
        throw Panic("domain is not the coset offset*<omega_n> in natural order (coset_fri.rs:32-36)");
    *offset = off;
    return log_n;
}
}  // namespace

// --------------------------------------------------------------- MerkleTree
MerkleTree::MerkleTree(const std::vector<FE>& data) {
    if (data.empty()) throw Panic("MerkleTree of no leaves has no root (merkle/mod.rs:25)");
    gpu_ = Gpu::thread_default(ceil_log2(data.size()));
    auto v = to_u32(data);
    uint8_t root[32];
    gpu_->check(fri_merkle_root(gpu_->ctx(), v.data(), v.size(), root), "fri_merkle_root");
    root_hex_ = sha::hex(root, 32);
    gpu_.reset();                                     // standalone: root only
}

std::array<uint8_t, 32> MerkleTree::root_bytes() const {
    auto b = sha::from_hex(root_hex_);
    std::array<uint8_t, 32> r{};
    std::memcpy(r.data(), b.data(), 32);
    return r;
}

std::vector<uint8_t> MerkleTree::get_authentication_path(size_t index) const {
    if (!gpu_) throw Panic("authentication paths are served by the trees of an FRIProof (standalone trees keep only the root)");
    if (gpu_->generation() != gen_) throw Panic("FRIProof layers were replaced by a later commit on the same Gpu");
    uint32_t value = 0, depth = 0;
    std::vector<uint8_t> path(32 * 32);
    if (member_ >= 0) {
        // a member of a batch: the opening of `index` in layer k is at index mod 2^(log_n - k) = index
        if (index >> (log_n_ - layer_)) throw Panic("authentication path: index out of range");
        size_t bytes = 0, off = 0, got = 0;
        for (uint32_t k = 0; k < n_layers_; k++) {
            if (k == layer_) off = bytes;
            bytes += 2 * 32 * size_t{log_n_ - k};
        }
        std::vector<uint32_t> values(2 * size_t{n_layers_});
        std::vector<uint8_t> paths(bytes ? bytes : 1);
        gpu_->check(fri_batch_decommit_query(gpu_->ctx(), static_cast<uint32_t>(member_), index, values.data(),
                                             values.size(), paths.data(), paths.size(), &got),
                    "fri_batch_decommit_query");
        const size_t pb = 32 * size_t{log_n_ - layer_};
        return std::vector<uint8_t>(paths.begin() + off, paths.begin() + off + pb);
    }
    gpu_->check(fri_auth_path(gpu_->ctx(), layer_, index, &value, path.data(), &depth), "fri_auth_path");
    path.resize(32 * size_t{depth});
    return path;
}

// ----------------------------------------------------------------- FRIProof
bool FRIProof::resident() const { return gpu_ && gpu_->generation() == gen_; }

void FRIProof::require_resident() const {
    if (!resident()) throw Panic("FRIProof layers were replaced by a later commit on the same Gpu");
}

std::vector<FE> FRIProof::fri_layer(size_t k) const {
    require_resident();
    if (k >= n_layers()) throw Panic("no such FRI layer");
    const size_t m = size_t{1} << (log_n - k);
    std::vector<uint32_t> v(m);
    if (member_ >= 0)
        gpu_->check(fri_batch_layer_copy(gpu_->ctx(), static_cast<uint32_t>(member_), static_cast<uint32_t>(k), v.data(), m),
                    "fri_batch_layer_copy");
    else
        gpu_->check(fri_layer_copy(gpu_->ctx(), static_cast<uint32_t>(k), v.data(), m), "fri_layer_copy");
    return to_fe(v.data(), m);
}

std::vector<std::vector<FE>> FRIProof::fri_layers() const {
    std::vector<std::vector<FE>> out;
    for (size_t k = 0; k < n_layers(); k++) out.push_back(fri_layer(k));
    return out;
}

// --------------------------------------------------------------- fri_commit
FRIProof fri_commit_coset(const Poly& poly, uint32_t log_n, FE offset, FriChannel& channel,
                          const std::shared_ptr<Gpu>& gpu) {
    if (!gpu) throw Panic("fri_commit: no Gpu");
    if (log_n > gpu->log_n_max()) throw Panic("fri_commit: codeword 2^" + std::to_string(log_n) + " exceeds the context");
    std::vector<uint32_t> coeffs = to_u32(poly.coefficients);
    fri_channel_state cin{};
    const fri_channel_state* pin = nullptr;
    if (!channel.state.empty()) {
        auto st = sha::from_hex(channel.state);
        if (st.size() != 32) throw Panic("Channel state is not a SHA-256 digest");
        std::memcpy(cin.digest, st.data(), 32);
        cin.has_state = 1;
        pin = &cin;
    }
    fri_commit_result res{};
    gpu->bump();                                    // previous layers are overwritten from here on
    gpu->check(fri_commit(gpu->ctx(), coeffs.data(), coeffs.size(), log_n, static_cast<uint32_t>(offset.value()), pin,
                          0, nullptr, &res),
               "fri_commit");

    return FRIProof::mirror(res, log_n, gpu, channel);
}

std::vector<FRIProof> fri_commit_pipelined(const std::vector<Poly>& polys, uint32_t log_n, FE offset,
                                           std::vector<FriChannel>& channels, const std::shared_ptr<Gpu>& gpu) {
    if (!gpu) throw Panic("fri_commit: no Gpu");
    if (channels.size() != polys.size()) throw Panic("fri_commit_pipelined: one channel per polynomial");
    if (log_n > gpu->log_n_max()) throw Panic("fri_commit: codeword 2^" + std::to_string(log_n) + " exceeds the context");
    struct Pending { size_t i; uint64_t ticket, gen; };
    std::vector<FRIProof> out(polys.size());
    std::vector<Pending> pend;
    auto collect = [&](const Pending& p) {
        fri_commit_result res{};
        gpu->check(fri_commit_wait(gpu->ctx(), p.ticket, &res), "fri_commit_wait");
        out[p.i] = FRIProof::mirror(res, log_n, gpu, channels[p.i], p.gen);
    };
    try {
        for (size_t i = 0; i < polys.size(); i++) {
            if (pend.size() == FRI_DEFAULT_LANES) {   // one pending commit per commit lane
                const Pending p = pend.front();
                pend.erase(pend.begin());   // waited below even if collect throws
                collect(p);
            }
            std::vector<uint32_t> coeffs = to_u32(polys[i].coefficients);
            fri_channel_state cin{};
            const fri_channel_state* pin = nullptr;
            if (!channels[i].state.empty()) {
                auto st = sha::from_hex(channels[i].state);
                if (st.size() != 32) throw Panic("Channel state is not a SHA-256 digest");
                std::memcpy(cin.digest, st.data(), 32);
                cin.has_state = 1;
                pin = &cin;
            }
            uint64_t ticket = 0;
            const uint64_t gen = gpu->bump();          // this commit's layers replace the previous ones
            gpu->check(fri_commit_async(gpu->ctx(), coeffs.data(), coeffs.size(), log_n,
                                        static_cast<uint32_t>(offset.value()), pin, 0, nullptr, &ticket),
                       "fri_commit_async");
            pend.push_back({i, ticket, gen});
        }
        while (!pend.empty()) {
            const Pending p = pend.front();
            pend.erase(pend.begin());
            collect(p);
        }
    } catch (...) {
        // a failed commit (reported at its wait) must not leave the other
        // result slots of this per-thread Gpu pending: wait for them all,
        // discarding their results, then re-throw
        for (const Pending& p : pend) {
            fri_commit_result res{};
            (void)fri_commit_wait(gpu->ctx(), p.ticket, &res);
        }
        throw;
    }
    return out;
}

std::vector<FRIProof> fri_commit_batch(const std::vector<Poly>& polys, uint32_t log_n, FE offset,
                                       std::vector<FriChannel>& channels, const std::shared_ptr<Gpu>& gpu) {
    if (channels.size() != polys.size()) throw Panic("fri_commit_batch: one channel per polynomial");
    if (polys.empty()) return {};
    if (!gpu) throw Panic("fri_commit: no Gpu");
    if (gpu->n_ranks() > 1) throw Panic("fri_commit_batch: batches run on a one-device Gpu");
    if (log_n > gpu->log_n_max()) throw Panic("fri_commit: codeword 2^" + std::to_string(log_n) + " exceeds the context");
    const size_t B = polys.size();
    size_t d = 0;
    for (const Poly& p : polys) d = std::max(d, p.coefficients.size());
    std::vector<uint32_t> coeffs(B * d, 0u);                 // ragged members: zeros up to the longest
    std::vector<fri_channel_state> cin(B);
    for (size_t b = 0; b < B; b++) {
        const std::vector<uint32_t> c = to_u32(polys[b].coefficients);
        std::copy(c.begin(), c.end(), coeffs.begin() + b * d);
        if (!channels[b].state.empty()) {
            auto st = sha::from_hex(channels[b].state);
            if (st.size() != 32) throw Panic("Channel state is not a SHA-256 digest");
            std::memcpy(cin[b].digest, st.data(), 32);
            cin[b].has_state = 1;
        }
    }
    std::vector<fri_commit_result> res(B);
    std::vector<int> status(B, 0);
    const uint64_t gen = gpu->bump();                        // previous layers are not served from here on
    gpu->check(fri_commit_batch(gpu->ctx(), coeffs.data(), d, static_cast<uint32_t>(B), log_n,
                                static_cast<uint32_t>(offset.value()), cin.data(), 0, nullptr, res.data(), status.data()),
               "fri_commit_batch");
    std::vector<FRIProof> out;
    for (size_t b = 0; b < B; b++) out.push_back(FRIProof::mirror_member(res[b], log_n, gpu, channels[b], gen, b));
    return out;
}

FRIProof FRIProof::mirror_member(const fri_commit_result& res, uint32_t log_n, const std::shared_ptr<Gpu>& gpu,
                                 FriChannel& channel, uint64_t gen, size_t member) {
    FRIProof proof = mirror(res, log_n, gpu, channel, gen);
    proof.member_ = static_cast<int>(member);
    for (MerkleTree& t : proof.fri_merkles) {
        t.member_ = proof.member_;
        t.log_n_ = log_n;
        t.n_layers_ = res.n_layers;
    }
    return proof;
}

FRIProof FRIProof::mirror(const fri_commit_result& res, uint32_t log_n, const std::shared_ptr<Gpu>& gpu,
                          FriChannel& channel, uint64_t gen) {
    // The channel messages the reference's loop produced (fri_commit.rs:84-114):
    // root_hex bytes per layer, beta (8 B BE, proof only) per round, final value.
    FRIProof proof;
    proof.log_n = log_n;
    proof.gpu_ = gpu;
    proof.gen_ = gen ? gen : gpu->generation();
    for (uint32_t k = 0; k < res.n_layers; k++) {
        const std::string hex = sha::hex(res.roots[k], 32);
        std::vector<uint8_t> msg(hex.begin(), hex.end());
        channel.proof.push_back(msg);
        channel.compressed_proof.push_back(msg);
        if (k < res.n_rounds) {
            channel.proof.push_back(FriChannel::be64(res.betas[k]));
            proof.betas.push_back(FE(res.betas[k]));
        }
        MerkleTree t;
        t.root_hex_ = hex;
        t.gpu_ = gpu;
        t.gen_ = proof.gen_;
        t.layer_ = k;
        proof.fri_merkles.push_back(std::move(t));
    }
    auto fv = FriChannel::be64(res.final_value);
    channel.proof.push_back(fv);
    channel.compressed_proof.push_back(fv);
    channel.state = res.channel_out.has_state ? sha::hex(res.channel_out.digest, 32) : "";
    proof.final_poly = res.final_degree < 0 ? Poly::zero() : Poly({FE(res.final_value)});
    return proof;
}

FRIProof fri_commit(Poly poly, std::vector<FE> domain, FriChannel& channel) {
    FE offset;
    const uint32_t log_n = coset_log_n(domain, &offset);
    domain.clear();
    domain.shrink_to_fit();
    return fri_commit_coset(poly, log_n, offset, channel, Gpu::thread_default(log_n));
}

FRIProof fri_commit(const Poly& poly, const Coset& coset, FriChannel& channel) {
    const size_t n = coset.domain_size;
    if (n == 0 || (n & (n - 1))) throw Panic("domain size must be a power of two");
    const uint32_t log_n = ceil_log2(n);
    if (coset.omega != omega(log_n)) throw Panic("coset omega must be g^((p-1)/n) (frozen spec)");
    if (coset.offset == FE::zero()) throw Panic("domain offset must be non-zero");
    return fri_commit_coset(poly, log_n, coset.offset, channel, Gpu::thread_default(log_n));
}

// ------------------------------------------------------------------ decommit
namespace {
// One query (decommit_fri_layers, fri_commit.rs:137-163) through the gather
// kernel on the commit resident on `gpu`: per layer send value, path,
// sibling value, sibling path (a 1-element layer sends its value first).
// `layers` (optional): the caller's FRIProof.fri_layers, checked against the
// device's openings.
void decommit_query(const Gpu& gpu, uint32_t log_n, size_t n_layers, uint64_t index, FriChannel& channel,
                    const std::vector<std::vector<FE>>* layers, int member = -1) {
    size_t path_bytes = 0;
    for (size_t k = 0; k < n_layers; k++) path_bytes += 2 * 32 * (log_n - k);
    std::vector<uint32_t> values(2 * n_layers);
    std::vector<uint8_t> paths(path_bytes ? path_bytes : 1);
    size_t got = 0;
    if (member >= 0)      // a member of the resident batch
        gpu.check(fri_batch_decommit_query(gpu.ctx(), static_cast<uint32_t>(member), index, values.data(), values.size(),
                                           paths.data(), paths.size(), &got),
                  "fri_batch_decommit_query");
    else
        gpu.check(fri_decommit_query(gpu.ctx(), index, values.data(), values.size(), paths.data(), paths.size(), &got),
                  "fri_decommit_query");
    size_t off = 0;
    for (size_t k = 0; k < n_layers; k++) {
        const size_t depth = log_n - k, pb = 32 * depth, m = size_t{1} << depth;
        if (layers) {
            const std::vector<FE>& lk = (*layers)[k];
            const size_t i = index % m, sib = (i + m / 2) % m;
            if (lk.size() != m || lk[i].value() != values[2 * k] || lk[sib].value() != values[2 * k + 1])
                throw Panic("fri_layers do not belong to the commit of these fri_merkles (layer " + std::to_string(k) +
                            ")");
        }
        std::vector<uint8_t> path(paths.begin() + off, paths.begin() + off + pb);
        std::vector<uint8_t> spath(paths.begin() + off + pb, paths.begin() + off + 2 * pb);
        off += 2 * pb;
        auto v = FE(values[2 * k]).to_bytes(), sv = FE(values[2 * k + 1]).to_bytes();
        if (depth == 0) channel.send(v);             // fri_commit.rs:147-149: length == 1 sends it first
        channel.send(v);
        channel.send(path);
        channel.send(sv);
        channel.send(spath);
    }
}
}  // namespace

void decommit_fri_layers(size_t index, const FRIProof& proof, FriChannel& channel) {
    proof.require_resident();
    decommit_query(*proof.gpu_, proof.log_n, proof.n_layers(), index, channel, nullptr, proof.member_);
}

void decommit_fri(size_t num_queries, size_t max_index, const FRIProof& proof, FriChannel& channel,
                  uint32_t grinding_bits) {
    grind_step(channel, grinding_bits, proof.gpu_);
    for (size_t q = 0; q < num_queries; q++) {
        const uint64_t idx = channel.receive_random_int(0, max_index, true);
        decommit_fri_layers(idx, proof, channel);
    }
}

namespace {
// The sizes of a query record (fri_batch_query_round, fri_amd.h, has the
// layout) of a member with `layers` layers: its values in words, its paths in
// bytes (trace_count of log_n digests, then layer k's two of log_n - k).
struct RecordShape {
    uint32_t log_n, trace_count;
    size_t val_words(size_t layers) const { return trace_count + 2 * layers; }
    size_t path_bytes(size_t layers) const {
        size_t n = size_t{trace_count} * 32 * log_n;
        for (size_t k = 0; k < layers; k++) n += 64 * (log_n - k);
        return n;
    }
};

// One record's messages in the transcript's order, each to sink(bytes, len):
// trace_count (value, path) pairs, then per layer (value, path, sibling value,
// sibling path) as decommit_query sends them, a one-element layer's value once
// more first (fri_commit.rs:147-149).
template <class Sink>
void walk_record(const uint32_t* values, const uint8_t* paths, const RecordShape& shape, size_t n_layers, Sink&& sink) {
    const size_t tc = shape.trace_count, tpath = 32 * size_t{shape.log_n};
    auto value = [&](uint32_t v) {
        const auto m = FriChannel::be64(v);
        sink(m.data(), m.size());
    };
    for (size_t j = 0; j < tc; j++) {
        value(values[j]);
        sink(paths + j * tpath, tpath);
    }
    size_t off = tc * tpath;
    for (size_t k = 0; k < n_layers; k++) {
        const size_t pb = 32 * size_t{shape.log_n - k};
        if (pb == 0) value(values[tc + 2 * k]);
        value(values[tc + 2 * k]);
        sink(paths + off, pb);
        value(values[tc + 2 * k + 1]);
        sink(paths + off + pb, pb);
        off += 2 * pb;
    }
}

// What both calls below start with: the resident batch has one member per
// channel (else `mismatch`), and the records' strides hold the most layers.
struct RecordStrides {
    RecordShape shape;
    size_t vstride, pstride;
};
RecordStrides record_strides(const Gpu& gpu, size_t B, const char* mismatch, uint32_t log_n,
                             const std::vector<size_t>& n_layers, uint32_t trace_count) {
    uint64_t generation = 0;
    uint32_t members = 0, resident_log_n = 0;
    gpu.check(fri_batch_info(gpu.ctx(), &generation, &members, &resident_log_n), "fri_batch_info");
    if (members != B) throw Panic(mismatch);
    size_t max_layers = 0;
    for (size_t nl : n_layers) max_layers = std::max(max_layers, nl);
    const RecordShape shape{log_n, trace_count};
    return {shape, shape.val_words(max_layers), std::max<size_t>(shape.path_bytes(max_layers), 1)};
}

// One fri_batch_query_round on `gpu` for members of `n_layers[b]` layers, then
// every channel absorbs its record (walk_record).
void query_round(const Gpu& gpu, uint32_t log_n, const std::vector<size_t>& n_layers,
                 const std::vector<uint64_t>& indices, uint32_t trace_count, uint64_t trace_stride,
                 std::vector<FriChannel>& channels) {
    const size_t B = channels.size();
    const auto [shape, vstride, pstride] = record_strides(
        gpu, B, "fri_batch_query_round: one index per member of the resident batch", log_n, n_layers, trace_count);
    std::vector<uint32_t> values(B * vstride);
    std::vector<uint8_t> paths(B * pstride);
    std::vector<size_t> got(B, 0);
    gpu.check(fri_batch_query_round(gpu.ctx(), indices.data(), nullptr, trace_count, trace_stride, values.data(), vstride,
                                    paths.data(), pstride, got.data()),
              "fri_batch_query_round");
    for (size_t b = 0; b < B; b++) {
        if (got[b] != shape.path_bytes(n_layers[b]))
            throw Panic("fri_batch_query_round: member " + std::to_string(b) + " was not served");
        FriChannel& ch = channels[b];
        walk_record(values.data() + b * vstride, paths.data() + b * pstride, shape, n_layers[b],
                    [&ch](const uint8_t* m, size_t len) { ch.send(m, len); });
    }
}

// The whole query phase of a batch in ONE fri_batch_query_phase: per member
// num_queries x (the drawn index, then the round's sends), run by the device
// on the member's channel.  Every channel then takes over its messages (an
// index goes to `proof` alone, as receive_random_int(.., true) leaves it) and
// its final state without hashing.  Returns the members' indices.
std::vector<std::vector<uint64_t>> query_phase(const Gpu& gpu, uint32_t log_n, const std::vector<size_t>& n_layers,
                                               size_t num_queries, uint64_t max_index, uint32_t trace_count,
                                               uint64_t trace_stride, std::vector<FriChannel>& channels) {
    const size_t B = channels.size(), Q = num_queries;
    std::vector<std::vector<uint64_t>> out(B);
    if (Q == 0) return out;
    const auto [shape, vstride, pstride] = record_strides(
        gpu, B, "fri_batch_query_phase: one channel per member of the resident batch", log_n, n_layers, trace_count);
    if (Q >> 32) throw Panic("fri_batch_query_phase: num_queries out of range");
    std::vector<fri_channel_state> chan(B);
    for (size_t b = 0; b < B; b++) {
        if (channels[b].state.size() != 64) throw Panic("Channel state is not valid hex");     // channel.rs:65
        auto st = sha::from_hex(channels[b].state);
        std::memcpy(chan[b].digest, st.data(), 32);
        chan[b].has_state = 1;
    }
    std::vector<uint64_t> indices(B * Q);
    std::vector<uint32_t> values(B * Q * vstride);
    std::vector<uint8_t> paths(B * Q * pstride);
    std::vector<size_t> got(B, 0);
    gpu.check(fri_batch_query_phase(gpu.ctx(), static_cast<uint32_t>(Q), max_index, chan.data(), nullptr, trace_count,
                                    trace_stride, indices.data(), values.data(), vstride, paths.data(), pstride,
                                    got.data()),
              "fri_batch_query_phase");
    for (size_t b = 0; b < B; b++) {
        if (got[b] != shape.path_bytes(n_layers[b]))
            throw Panic("fri_batch_query_phase: member " + std::to_string(b) + " was not served");
        FriChannel& ch = channels[b];
        auto put = [&ch](const uint8_t* m, size_t len) {
            ch.compressed_proof.emplace_back(m, m + len);
            ch.proof.emplace_back(m, m + len);
        };
        for (size_t q = 0; q < Q; q++) {
            out[b].push_back(indices[b * Q + q]);
            ch.proof.push_back(FriChannel::be64(indices[b * Q + q]));
            walk_record(values.data() + (b * Q + q) * vstride, paths.data() + (b * Q + q) * pstride, shape, n_layers[b],
                        put);
        }
        ch.state = sha::hex(chan[b].digest, 32);
    }
    return out;
}
}  // namespace

void decommit_fri_batch(size_t num_queries, size_t max_index, const std::vector<FRIProof>& proofs,
                        std::vector<FriChannel>& channels, bool device_queries, uint32_t grinding_bits) {
    check_grinding_bits(grinding_bits);
    if (channels.size() != proofs.size()) throw Panic("decommit_fri_batch: one channel per proof");
    if (proofs.empty()) return;
    const FRIProof& p0 = proofs[0];
    std::vector<size_t> n_layers;
    for (size_t b = 0; b < proofs.size(); b++) {
        const FRIProof& p = proofs[b];
        if (p.gpu_ != p0.gpu_ || p.gen_ != p0.gen_ || p.log_n != p0.log_n || p.member_ != static_cast<int>(b))
            throw Panic("decommit_fri_batch: the proofs are not the members of one batch, in member order");
        n_layers.push_back(p.n_layers());
    }
    p0.require_resident();
    grind_step_batch(channels, grinding_bits, *p0.gpu_);
    if (device_queries) {
        query_phase(*p0.gpu_, p0.log_n, n_layers, num_queries, max_index, 0, 0, channels);
        return;
    }
    std::vector<uint64_t> idx(proofs.size());
    for (size_t q = 0; q < num_queries; q++) {
        for (size_t b = 0; b < proofs.size(); b++) idx[b] = channels[b].receive_random_int(0, max_index, true);
        query_round(*p0.gpu_, p0.log_n, n_layers, idx, 0, 0, channels);
    }
}

void decommit_fri(size_t num_queries, size_t max_index, const std::vector<std::vector<FE>>& fri_layers,
                  const std::vector<MerkleTree>& fri_merkles, FriChannel& channel, uint32_t grinding_bits) {
    if (fri_merkles.empty()) throw Panic("decommit_fri: no FRI layers");
    if (fri_layers.size() != fri_merkles.size()) throw Panic("decommit_fri: one Merkle tree per FRI layer");
    const MerkleTree& t0 = fri_merkles[0];
    if (!t0.gpu_) throw Panic("decommit_fri: the trees of an FRIProof are device-backed; a standalone tree keeps only its root");
    for (size_t k = 0; k < fri_merkles.size(); k++) {
        const MerkleTree& t = fri_merkles[k];
        if (t.gpu_ != t0.gpu_ || t.gen_ != t0.gen_ || t.layer_ != k || t.member_ != t0.member_)
            throw Panic("decommit_fri: the trees are not the layers of one commit");
    }
    const Gpu& gpu = *t0.gpu_;
    if (gpu.generation() != t0.gen_) throw Panic("FRIProof layers were replaced by a later commit on the same Gpu");
    uint64_t g = 0;
    uint32_t log_n = 0, n_layers = 0;
    if (t0.member_ >= 0) {        // a member of a batch: its shape travels with its trees
        uint32_t members = 0;
        gpu.check(fri_batch_info(gpu.ctx(), &g, &members, &log_n), "fri_batch_info");
        n_layers = static_cast<uint32_t>(t0.member_) < members && log_n == t0.log_n_ ? t0.n_layers_ : 0;
    } else {
        gpu.check(fri_commit_info(gpu.ctx(), &g, &log_n, &n_layers), "fri_commit_info");
    }
    if (n_layers != fri_merkles.size() || fri_layers[0].size() != (size_t{1} << log_n))
        throw Panic("decommit_fri: the resident commit is not the one these trees belong to");
    grind_step(channel, grinding_bits, t0.gpu_);
    for (size_t q = 0; q < num_queries; q++) {
        const uint64_t idx = channel.receive_random_int(0, max_index, true);
        decommit_query(gpu, log_n, n_layers, idx, channel, &fri_layers, t0.member_);
    }
}

// -------------------------------------------------------------------- verify
namespace {
bool path_ok(uint64_t value, uint64_t index, const std::vector<uint8_t>& path, size_t depth,
             const std::array<uint8_t, 32>& root) {
    if (path.size() != 32 * depth) return false;
    const auto leaf = FE(value).to_bytes();                     // merkle/mod.rs:14-15
    auto h = sha::digest(leaf.data(), 8);
    uint8_t buf[64];
    for (size_t lvl = 0; lvl < depth; lvl++) {
        const uint8_t* sib = path.data() + 32 * lvl;
        if ((index >> lvl) & 1) {
            std::memcpy(buf, sib, 32);
            std::memcpy(buf + 32, h.data(), 32);
        } else {
            std::memcpy(buf, h.data(), 32);
            std::memcpy(buf + 32, sib, 32);
        }
        h = sha::digest(buf, 64);
    }
    return h == root;
}

uint64_t be_u64(const std::vector<uint8_t>& b) {
    uint64_t v = 0;
    for (uint8_t c : b) v = v << 8 | c;
    return v;
}
}  // namespace

namespace {
using Msgs = std::vector<std::vector<uint8_t>>;
using Take = std::function<const std::vector<uint8_t>&()>;
// verify_fri's replay with two hooks for a STARK around the FRI:
// pre_commit consumes the messages before the first FRI root; on_query those
// between a query index and its layer openings and returns the value layer 0
// must hold there (or -1).  A hook rejects by throwing Panic.
bool verify_transcript(const Msgs& msgs, uint32_t log_n, size_t n_layers, size_t num_queries, size_t max_index,
                       FE offset, const std::string& channel_state,
                       const std::function<void(const Take&, FriChannel&)>& pre_commit,
                       const std::function<int64_t(const Take&, FriChannel&, uint64_t)>& on_query,
                       uint32_t grinding_bits) {
    check_grinding_bits(grinding_bits);
    if (n_layers == 0 || n_layers > log_n + 1u) return false;
    size_t pos = 0;
    Take take = [&]() -> const std::vector<uint8_t>& {
        if (pos >= msgs.size()) throw Panic("transcript ended early");
        return msgs[pos++];
    };
    try {
        FriChannel ch;
        ch.state = channel_state;
        if (pre_commit) pre_commit(take, ch);
        std::vector<std::array<uint8_t, 32>> roots;
        std::vector<FE> betas;
        for (size_t k = 0; k < n_layers; k++) {
            const auto& r = take();
            if (r.size() != 64) return false;
            auto rb = sha::from_hex(std::string(r.begin(), r.end()));
            std::array<uint8_t, 32> ra{};
            std::memcpy(ra.data(), rb.data(), 32);
            roots.push_back(ra);
            ch.send(r);
            if (k + 1 < n_layers) {
                FE beta = ch.receive_random_field_element();
                if (take() != FriChannel::be64(beta.value())) return false;
                betas.push_back(beta);
            }
        }
        const auto& fin = take();
        if (fin.size() != 8) return false;
        const uint64_t final_value = be_u64(fin);
        ch.send(fin);
        if (grinding_bits) {
            const auto& nonce = take();
            if (nonce.size() != 8) return false;
            ch.send(nonce);
            if (!state_has_zero_bits(ch.state, grinding_bits)) return false;
        }
        const FE inv2 = FE(2).inverse();
        for (size_t q = 0; q < num_queries; q++) {
            const uint64_t idx = ch.receive_random_int(0, max_index, true);
            if (take() != FriChannel::be64(idx)) return false;
            const int64_t want0 = on_query ? on_query(take, ch, idx) : -1;
            bool have_prev = false;
            uint64_t pa = 0, pb = 0, pj = 0, pm = 0;           // L[pj], L[pj + pm/2] of layer k-1
            for (size_t k = 0; k < n_layers; k++) {
                const size_t depth = log_n - k;
                const uint64_t m = uint64_t{1} << depth;
                const std::vector<uint8_t>* extra = nullptr;
                if (m == 1) {                                    // fri_commit.rs:147-149 sends layer[0] first
                    extra = &take();
                    ch.send(*extra);
                }
                const uint64_t i = idx % m, sib = (i + m / 2) % m;
                const auto& vb = take();
                if (extra && *extra != vb) return false;
                const auto& path = take();
                const auto& sb = take();
                const auto& spath = take();
                for (auto* msg : {&vb, &path, &sb, &spath}) ch.send(*msg);
                if (vb.size() != 8 || sb.size() != 8) return false;
                const uint64_t v = be_u64(vb), sv = be_u64(sb);
                if (v >= P || sv >= P) return false;
                if (!path_ok(v, i, path, depth, roots[k]) || !path_ok(sv, sib, spath, depth, roots[k])) return false;
                if (k == 0 && want0 >= 0 && v != static_cast<uint64_t>(want0)) return false;
                if (have_prev) {
                    // x = offset^(2^(k-1)) * omega_pm^pj; fold = (a+b)/2 + beta*(a-b)/(2x)  (fri_commit.rs:32-65)
                    const FE x = offset.pow(uint64_t{1} << (k - 1)) * omega(ceil_log2(pm)).pow(pj);
                    const FE a(pa), b(pb);
                    const FE fold = ((a + b) + betas[k - 1] * (a - b) * x.inverse()) * inv2;
                    if (fold.value() != v) return false;
                }
                const uint64_t j = m > 1 ? i % (m / 2) : 0;
                if (i < m / 2 || m == 1) { pa = v; pb = sv; } else { pa = sv; pb = v; }
                pj = j;
                pm = m;
                have_prev = true;
                if (k + 1 == n_layers && (v != final_value || sv != final_value)) return false;
            }
        }
        return pos == msgs.size();
    } catch (const Panic&) {
        return false;
    }
}
}  // namespace

bool verify_fri(const Msgs& msgs, uint32_t log_n, size_t n_layers, size_t num_queries, size_t max_index, FE offset,
                const std::string& channel_state, uint32_t grinding_bits) {
    return verify_transcript(msgs, log_n, n_layers, num_queries, max_index, offset, channel_state, nullptr, nullptr,
                             grinding_bits);
}

// ----------------------------------------------------------- prover slice
std::vector<FE> fibsq_trace(FE a1, uint32_t log_t) {
    std::vector<uint32_t> t(size_t{1} << log_t);
    if (fri_fibsq_trace(static_cast<uint32_t>(a1.value()), log_t, t.data()) != FRI_OK) throw Panic("fri_fibsq_trace");
    return to_fe(t.data(), t.size());
}

StarkProof prove_fibsq(FE a1, uint32_t log_t, uint32_t log_blowup, size_t num_queries, FriChannel& channel, FE offset,
                       std::shared_ptr<Gpu> gpu, uint32_t grinding_bits) {
    check_grinding_bits(grinding_bits);
    const uint32_t L = log_t + log_blowup;
    const uint64_t B = uint64_t{1} << log_blowup, n = uint64_t{1} << L;
    if (!gpu) gpu = Gpu::thread_default(L);
    if (L > gpu->log_n_max()) throw Panic("prove_fibsq: LDE 2^" + std::to_string(L) + " exceeds the context");
    std::vector<uint32_t> trace(size_t{1} << log_t);
    gpu->check(fri_fibsq_trace(static_cast<uint32_t>(a1.value()), log_t, trace.data()), "fri_fibsq_trace");
    StarkProof sp;
    sp.log_t = log_t;
    sp.log_blowup = log_blowup;
    sp.a_last = FE(trace.back());
    const uint32_t off = static_cast<uint32_t>(offset.value());
    gpu->check(fri_trace_commit(gpu->ctx(), trace.data(), log_t, log_blowup, off, sp.trace_root.data(), nullptr,
                                nullptr, nullptr),
               "fri_trace_commit");
    const std::string root_hex = sha::hex(sp.trace_root.data(), 32);
    channel.send(reinterpret_cast<const uint8_t*>(root_hex.data()), root_hex.size());
    for (auto& a : sp.alphas) a = channel.receive_random_field_element();
    fri_channel_state cin{};
    auto st = sha::from_hex(channel.state);
    std::memcpy(cin.digest, st.data(), 32);
    cin.has_state = 1;
    const uint32_t al[3] = {static_cast<uint32_t>(sp.alphas[0].value()), static_cast<uint32_t>(sp.alphas[1].value()),
                            static_cast<uint32_t>(sp.alphas[2].value())};
    fri_commit_result res{};
    gpu->bump();
    gpu->check(fri_fibsq_composition_commit(gpu->ctx(), log_t, log_blowup, off, trace.back(), al, &cin, 0, &res),
               "fri_fibsq_composition_commit");
    sp.fri = FRIProof::mirror(res, L, gpu, channel);
    grind_step(channel, grinding_bits, gpu);
    std::vector<uint32_t> vals(3);
    std::vector<uint8_t> paths(3 * 32 * size_t{L});
    for (size_t q = 0; q < num_queries; q++) {
        const uint64_t idx = channel.receive_random_int(0, n - 2 * B - 1, true);
        sp.queries.push_back(idx);
        gpu->check(fri_trace_decommit(gpu->ctx(), idx, B, 3, vals.data(), paths.data(), paths.size()),
                   "fri_trace_decommit");
        for (size_t j = 0; j < 3; j++) {
            channel.send(FE(vals[j]).to_bytes());
            channel.send(paths.data() + 32 * L * j, 32 * size_t{L});
        }
        decommit_fri_layers(idx, sp.fri, channel);
    }
    return sp;
}

namespace {
// The one-device Gpu of the batched calls beside a default team: per thread,
// on the team's first device (FRI_DEVICES' first entry, else device 0).
std::shared_ptr<Gpu> beside_team(uint32_t log_n) {
    static thread_local std::shared_ptr<Gpu> g;
    const uint32_t want = log_n < 12 ? 12 : log_n;
    if (!g || g->log_n_max() < want) {
        const char* e = std::getenv("FRI_DEVICES");
        g = std::make_shared<Gpu>(e && *e ? std::atoi(e) : 0, want);
    }
    return g;
}
}  // namespace

std::vector<StarkProof> prove_fibsq_batch(const std::vector<FE>& a1, uint32_t log_t, uint32_t log_blowup,
                                          size_t num_queries, std::vector<FriChannel>& channels, FE offset,
                                          std::shared_ptr<Gpu> gpu, bool device_queries, uint32_t grinding_bits) {
    check_grinding_bits(grinding_bits);
    if (channels.size() != a1.size()) throw Panic("prove_fibsq_batch: one channel per proof");
    if (a1.empty()) return {};
    const uint32_t L = log_t + log_blowup;
    const uint64_t Bl = uint64_t{1} << log_blowup, n = uint64_t{1} << L;
    const size_t B = a1.size(), T = size_t{1} << log_t;
    if (!gpu) {
        gpu = Gpu::thread_default(L);
        if (gpu->n_ranks() > 1) gpu = beside_team(L);        // batches run on one device
    }
    if (gpu->n_ranks() > 1) throw Panic("prove_fibsq_batch: batches run on a one-device Gpu");
    if (L > gpu->log_n_max()) throw Panic("prove_fibsq_batch: LDE 2^" + std::to_string(L) + " exceeds the context");
    const uint32_t off = static_cast<uint32_t>(offset.value());
    std::vector<uint32_t> traces(B * T), a_last(B), alphas(3 * B);
    for (size_t b = 0; b < B; b++) {
        gpu->check(fri_fibsq_trace(static_cast<uint32_t>(a1[b].value()), log_t, traces.data() + b * T), "fri_fibsq_trace");
        a_last[b] = traces[b * T + T - 1];
    }
    std::vector<uint8_t> roots(32 * B);
    gpu->check(fri_trace_commit_batch(gpu->ctx(), traces.data(), log_t, log_blowup, off, static_cast<uint32_t>(B),
                                      roots.data()),
               "fri_trace_commit_batch");
    std::vector<StarkProof> out(B);
    std::vector<fri_channel_state> cin(B);
    for (size_t b = 0; b < B; b++) {
        StarkProof& sp = out[b];
        sp.log_t = log_t;
        sp.log_blowup = log_blowup;
        sp.a_last = FE(a_last[b]);
        std::memcpy(sp.trace_root.data(), roots.data() + 32 * b, 32);
        const std::string root_hex = sha::hex(sp.trace_root.data(), 32);
        channels[b].send(reinterpret_cast<const uint8_t*>(root_hex.data()), root_hex.size());
        for (size_t j = 0; j < 3; j++) {
            sp.alphas[j] = channels[b].receive_random_field_element();
            alphas[3 * b + j] = static_cast<uint32_t>(sp.alphas[j].value());
        }
        auto st = sha::from_hex(channels[b].state);
        std::memcpy(cin[b].digest, st.data(), 32);
        cin[b].has_state = 1;
    }
    std::vector<fri_commit_result> res(B);
    std::vector<int> status(B, 0);
    const uint64_t gen = gpu->bump();
    gpu->check(fri_fibsq_composition_commit_batch(gpu->ctx(), log_t, log_blowup, off, static_cast<uint32_t>(B),
                                                  a_last.data(), alphas.data(), cin.data(), 0, res.data(),
                                                  status.data()),
               "fri_fibsq_composition_commit_batch");
    std::vector<size_t> n_layers(B);
    for (size_t b = 0; b < B; b++) {
        out[b].fri = FRIProof::mirror_member(res[b], L, gpu, channels[b], gen, b);
        n_layers[b] = res[b].n_layers;
    }
    grind_step_batch(channels, grinding_bits, *gpu);
    if (device_queries) {
        auto drawn = query_phase(*gpu, L, n_layers, num_queries, n - 2 * Bl - 1, 3, Bl, channels);
        for (size_t b = 0; b < B; b++) out[b].queries = std::move(drawn[b]);
        return out;
    }
    std::vector<uint64_t> idx(B);
    for (size_t q = 0; q < num_queries; q++) {
        for (size_t b = 0; b < B; b++) {
            idx[b] = channels[b].receive_random_int(0, n - 2 * Bl - 1, true);
            out[b].queries.push_back(idx[b]);
        }
        query_round(*gpu, L, n_layers, idx, 3, Bl, channels);
    }
    return out;
}

FE fibsq_composition_at(FE f0, FE f1, FE f2, FE x, const std::array<FE, 3>& alphas, FE a_last, uint32_t log_t) {
    const uint64_t T = uint64_t{1} << log_t;
    const FE g = omega(log_t), glast = g.pow(T - 1), gprev = g.pow(T - 2);
    const FE p0 = (f0 - FE(1)) * (x - FE(1)).inverse();
    const FE p1 = (f0 - a_last) * (x - glast).inverse();
    const FE p2 = (f2 - f1 * f1 - f0 * f0) * (x - gprev) * (x - glast) * (x.pow(T) - FE(1)).inverse();
    return alphas[0] * p0 + alphas[1] * p1 + alphas[2] * p2;
}

bool verify_fibsq(const Msgs& msgs, FE a_last, uint32_t log_t, uint32_t log_blowup, size_t num_queries,
                  size_t n_layers, FE offset, const std::string& channel_state, uint32_t grinding_bits) {
    const uint32_t L = log_t + log_blowup;
    const uint64_t B = uint64_t{1} << log_blowup, n = uint64_t{1} << L;
    std::array<uint8_t, 32> root{};
    std::array<FE, 3> alphas{};
    auto pre = [&](const Take& take, FriChannel& ch) {
        const auto& r = take();
        if (r.size() != 64) throw Panic("trace root");
        auto rb = sha::from_hex(std::string(r.begin(), r.end()));
        std::memcpy(root.data(), rb.data(), 32);
        ch.send(r);
        for (auto& a : alphas) {
            a = ch.receive_random_field_element();
            if (take() != FriChannel::be64(a.value())) throw Panic("alpha");
        }
    };
    auto on_query = [&](const Take& take, FriChannel& ch, uint64_t idx) -> int64_t {
        FE f[3];
        for (int j = 0; j < 3; j++) {
            const auto& vb = take();
            const auto& path = take();
            ch.send(vb);
            ch.send(path);
            if (vb.size() != 8) throw Panic("trace value");
            const uint64_t v = be_u64(vb);
            if (v >= P || !path_ok(v, idx + j * B, path, L, root)) throw Panic("trace path");
            f[j] = FE(v);
        }
        const FE x = offset * omega(L).pow(idx);
        return static_cast<int64_t>(fibsq_composition_at(f[0], f[1], f[2], x, alphas, a_last, log_t).value());
    };
    return verify_transcript(msgs, L, n_layers, num_queries, n - 2 * B - 1, offset, channel_state, pre, on_query,
                             grinding_bits);
}

// ------------------------------------------------------- batched verifier
namespace {
// Transcripts of one shape in fri_verify_batch's record layout (fri_amd.h).
struct Packed {
    fri_verify_shape sh{};
    size_t hw = 0, vw = 0, pb = 0;             // head words, values words, paths bytes per record
    std::vector<fri_channel_state> chan;
    std::vector<uint32_t> n_layers, a_last, head, values;
    std::vector<uint64_t> indices;
    std::vector<uint8_t> paths;
    std::vector<uint32_t> reasons;             // a host decision (FRI_VERIFY_MALFORMED) or 0
    std::vector<uint8_t> host;                 // 1: left to the host verifier
    uint32_t grinding_bits = 0;                // > 0: the message after the final value is the member's nonce
    std::vector<uint64_t> nonces;              // per member (zeros without grinding bits)
};
enum class PackRc { Ok, Malformed, Host };

bool canonical_hex(const std::vector<uint8_t>& m) {
    for (uint8_t c : m)
        if (!((c >= '0' && c <= '9') || (c >= 'a' && c <= 'f'))) return false;
    return true;
}

// Member b's messages into its records.  Malformed: what verify_transcript
// certainly rejects (a wrong message count for n_layers, a message of the
// wrong length, a value, challenge or final value >= p, a one-element layer
// whose doubled value differs).  Host: a root message that is not canonical
// lowercase hex cannot be packed as raw bytes (and a final value >= p that no
// query compares): the host verifier decides.  With grinding bits one more
// message, the nonce after the final value, which must be 8 bytes.
PackRc pack_member(Packed& pk, size_t b, const Msgs& msgs, size_t nl, const std::string& state) {
    const uint32_t L = pk.sh.log_n, ML = pk.sh.max_layers, Q = pk.sh.num_queries, tc = pk.sh.trace_count;
    if (nl == 0 || nl > L + 1u) return PackRc::Malformed;
    size_t per_q = 1 + 2 * tc;
    for (size_t k = 0; k < nl; k++) per_q += (L - k == 0) ? 5 : 4;
    if (msgs.size() != (tc ? 4 : 0) + 2 * nl + (pk.grinding_bits ? 1 : 0) + Q * per_q) return PackRc::Malformed;
    const size_t hb = tc ? 11 : 0;
    uint32_t* head = pk.head.data() + b * pk.hw;
    size_t pos = 0;
    bool malformed = false, to_host = false;
    auto value = [&](uint32_t& out) {
        const auto& m = msgs[pos++];
        const uint64_t v = m.size() == 8 ? be_u64(m) : P;
        if (v >= P) malformed = true;
        else out = static_cast<uint32_t>(v);
    };
    auto root = [&](uint32_t* out) {
        const auto& m = msgs[pos++];
        if (m.size() != 64) { malformed = true; return; }
        if (!canonical_hex(m)) { to_host = true; return; }
        const auto raw = sha::from_hex(std::string(m.begin(), m.end()));
        for (int i = 0; i < 8; i++)
            out[i] = uint32_t{raw[4 * i]} << 24 | uint32_t{raw[4 * i + 1]} << 16 | uint32_t{raw[4 * i + 2]} << 8 | raw[4 * i + 3];
    };
    if (tc) {
        root(head);
        for (int j = 0; j < 3; j++) value(head[8 + j]);
    }
    for (size_t k = 0; k < nl; k++) {
        root(head + hb + 8 * k);
        if (k + 1 < nl) value(head[hb + 8 * ML + k]);
    }
    if (Q == 0 && msgs[pos].size() == 8 && be_u64(msgs[pos]) >= P) to_host = true;
    value(head[hb + 9 * ML - 1]);
    if (pk.grinding_bits) {
        const auto& nm = msgs[pos++];
        if (nm.size() != 8) malformed = true;
        else pk.nonces[b] = be_u64(nm);
    }
    for (size_t q = 0; q < Q; q++) {
        const auto& im = msgs[pos++];
        if (im.size() != 8) malformed = true;
        else pk.indices[b * Q + q] = be_u64(im);
        uint32_t* vals = pk.values.data() + (b * Q + q) * pk.vw;
        uint8_t* rec = pk.paths.data() + (b * Q + q) * pk.pb;
        size_t off = 0;
        auto path = [&](size_t depth) {
            const auto& m = msgs[pos++];
            if (m.size() != 32 * depth) { malformed = true; return; }
            if (!m.empty()) std::memcpy(rec + off, m.data(), m.size());
            off += 32 * depth;
        };
        for (size_t j = 0; j < tc; j++) {
            value(vals[j]);
            path(L);
        }
        for (size_t k = 0; k < nl; k++) {
            const size_t depth = L - k;
            if (depth == 0 && msgs[pos] != msgs[pos + 1]) malformed = true;
            if (depth == 0) pos++;
            value(vals[tc + 2 * k]);
            path(depth);
            value(vals[tc + 2 * k + 1]);
            path(depth);
        }
    }
    if (malformed) return PackRc::Malformed;       // certain, whatever else the transcript holds
    if (to_host) return PackRc::Host;
    if (!state.empty()) {
        const auto st = sha::from_hex(state);
        if (st.size() != 32) throw Panic("verify batch: a channel state is \"\" or 64 hex characters");
        std::memcpy(pk.chan[b].digest, st.data(), 32);
        pk.chan[b].has_state = 1;
    }
    pk.n_layers[b] = static_cast<uint32_t>(nl);
    return PackRc::Ok;
}

Packed pack_batch(const std::vector<Msgs>& t, uint32_t log_n, const std::vector<size_t>& n_layers, size_t num_queries,
                  size_t max_index, uint32_t tc, uint32_t log_t, uint32_t log_blowup, FE offset,
                  const std::vector<std::string>& states, uint32_t grinding_bits) {
    const size_t B = t.size();
    Packed pk;
    pk.grinding_bits = grinding_bits;
    pk.nonces.assign(B, 0);
    size_t ML = 1;
    for (size_t nl : n_layers)
        if (nl <= log_n + 1u) ML = std::max(ML, nl);
    pk.sh.log_n = log_n;
    pk.sh.max_layers = static_cast<uint32_t>(ML);
    pk.sh.num_queries = static_cast<uint32_t>(num_queries);
    pk.sh.trace_count = tc;
    pk.sh.log_t = log_t;
    pk.sh.log_blowup = log_blowup;
    pk.sh.offset = static_cast<uint32_t>(offset.value());
    pk.sh.max_index = max_index;
    pk.hw = (tc ? 11 : 0) + 9 * ML;
    pk.vw = RecordShape{log_n, tc}.val_words(ML);
    pk.pb = RecordShape{log_n, tc}.path_bytes(ML);
    const size_t Q = num_queries;
    pk.chan.assign(B, fri_channel_state{});
    pk.n_layers.assign(B, 1);
    pk.a_last.assign(B, 0);
    pk.head.assign(B * pk.hw, 0);
    pk.values.assign(B * Q * pk.vw + 1, 0);
    pk.indices.assign(B * Q + 1, 0);
    pk.paths.assign(B * Q * pk.pb + 1, 0);
    pk.reasons.assign(B, 0);
    pk.host.assign(B, 0);
    for (size_t b = 0; b < B; b++) {
        const PackRc rc = pack_member(pk, b, t[b], n_layers[b], states.empty() ? std::string() : states[b]);
        if (rc == PackRc::Ok) continue;
        // a member decided on the host holds zeros and one layer
        std::fill(pk.head.begin() + b * pk.hw, pk.head.begin() + (b + 1) * pk.hw, 0u);
        std::fill(pk.values.begin() + b * Q * pk.vw, pk.values.begin() + (b + 1) * Q * pk.vw, 0u);
        std::fill(pk.indices.begin() + b * Q, pk.indices.begin() + (b + 1) * Q, uint64_t{0});
        std::fill(pk.paths.begin() + b * Q * pk.pb, pk.paths.begin() + (b + 1) * Q * pk.pb, uint8_t{0});
        pk.nonces[b] = 0;
        if (rc == PackRc::Malformed) pk.reasons[b] = FRI_VERIFY_MALFORMED;
        else pk.host[b] = 1;
    }
    return pk;
}

// The masks of a packed batch: the packer's decisions, host_verify(b) for the
// members it left to the host verifier, the device's for every other member.
std::vector<bool> verify_packed(Packed& pk, const std::function<bool(size_t)>& host_verify, std::shared_ptr<Gpu> gpu,
                                std::vector<uint32_t>* reasons, const char* what) {
    const size_t B = pk.reasons.size(), Q = pk.sh.num_queries;
    std::vector<uint32_t> mask = pk.reasons;
    bool device = false;
    for (size_t b = 0; b < B; b++) device = device || (!pk.reasons[b] && !pk.host[b]);
    if (device) {
        const uint32_t L = pk.sh.log_n;
        if (!gpu) {
            gpu = Gpu::thread_default(L);
            if (gpu->n_ranks() > 1) gpu = beside_team(L);        // the verifier runs on one device
        }
        if (gpu->n_ranks() > 1) throw Panic(std::string(what) + ": batches run on a one-device Gpu");
        if (L > gpu->log_n_max()) throw Panic(std::string(what) + ": 2^" + std::to_string(L) + " exceeds the context");
        std::vector<uint32_t> got(B, 0);
        for (size_t b0 = 0; b0 < B; b0 += 65535) {
            const size_t m = std::min<size_t>(65535, B - b0);
            const uint32_t* alast = pk.sh.trace_count ? pk.a_last.data() + b0 : nullptr;
            const uint32_t mm = static_cast<uint32_t>(m);
            const size_t ps = std::max<size_t>(pk.pb, 1);
            if (pk.grinding_bits)
                gpu->check(fri_verify_batch_pow(gpu->ctx(), &pk.sh, mm, pk.chan.data() + b0, pk.n_layers.data() + b0,
                                                alast, pk.head.data() + b0 * pk.hw, pk.hw, pk.indices.data() + b0 * Q,
                                                pk.values.data() + b0 * Q * pk.vw, pk.vw,
                                                pk.paths.data() + b0 * Q * pk.pb, ps, pk.grinding_bits,
                                                pk.nonces.data() + b0, got.data() + b0),
                           "fri_verify_batch_pow");
            else
                gpu->check(fri_verify_batch(gpu->ctx(), &pk.sh, mm, pk.chan.data() + b0, pk.n_layers.data() + b0,
                                            alast, pk.head.data() + b0 * pk.hw, pk.hw, pk.indices.data() + b0 * Q,
                                            pk.values.data() + b0 * Q * pk.vw, pk.vw,
                                            pk.paths.data() + b0 * Q * pk.pb, ps, got.data() + b0),
                           "fri_verify_batch");
        }
        for (size_t b = 0; b < B; b++)
            if (!pk.reasons[b] && !pk.host[b]) mask[b] = got[b];
    }
    for (size_t b = 0; b < B; b++)
        if (pk.host[b]) mask[b] = host_verify(b) ? 0u : uint32_t{FRI_VERIFY_MALFORMED};
    if (reasons) *reasons = mask;
    std::vector<bool> ok(B);
    for (size_t b = 0; b < B; b++) ok[b] = mask[b] == 0;
    return ok;
}
}  // namespace

std::vector<bool> verify_fri_batch(const std::vector<Msgs>& transcripts, uint32_t log_n,
                                   const std::vector<size_t>& n_layers, size_t num_queries, size_t max_index, FE offset,
                                   const std::vector<std::string>& channel_states, std::shared_ptr<Gpu> gpu,
                                   std::vector<uint32_t>* reasons, uint32_t grinding_bits) {
    check_grinding_bits(grinding_bits);
    const size_t B = transcripts.size();
    if (n_layers.size() != B || (!channel_states.empty() && channel_states.size() != B))
        throw Panic("verify_fri_batch: one n_layers and channel state per transcript");
    if (reasons) reasons->clear();
    if (B == 0) return {};
    Packed pk = pack_batch(transcripts, log_n, n_layers, num_queries, max_index, 0, 0, 0, offset, channel_states,
                           grinding_bits);
    auto host = [&](size_t b) {
        return verify_fri(transcripts[b], log_n, n_layers[b], num_queries, max_index, offset,
                          channel_states.empty() ? std::string() : channel_states[b], grinding_bits);
    };
    return verify_packed(pk, host, std::move(gpu), reasons, "verify_fri_batch");
}

std::vector<bool> verify_fibsq_batch(const std::vector<Msgs>& transcripts, const std::vector<FE>& a_last,
                                     uint32_t log_t, uint32_t log_blowup, size_t num_queries,
                                     const std::vector<size_t>& n_layers, FE offset,
                                     const std::vector<std::string>& channel_states, std::shared_ptr<Gpu> gpu,
                                     std::vector<uint32_t>* reasons, uint32_t grinding_bits) {
    check_grinding_bits(grinding_bits);
    const size_t B = transcripts.size();
    if (a_last.size() != B || n_layers.size() != B || (!channel_states.empty() && channel_states.size() != B))
        throw Panic("verify_fibsq_batch: one a_last, n_layers and channel state per transcript");
    if (reasons) reasons->clear();
    if (B == 0) return {};
    const uint32_t L = log_t + log_blowup;
    const size_t max_index = (size_t{1} << L) - 2 * (size_t{1} << log_blowup) - 1;
    Packed pk = pack_batch(transcripts, L, n_layers, num_queries, max_index, 3, log_t, log_blowup, offset, channel_states,
                           grinding_bits);
    for (size_t b = 0; b < B; b++) pk.a_last[b] = static_cast<uint32_t>(a_last[b].value());
    auto host = [&](size_t b) {
        return verify_fibsq(transcripts[b], a_last[b], log_t, log_blowup, num_queries, n_layers[b], offset,
                            channel_states.empty() ? std::string() : channel_states[b], grinding_bits);
    };
    return verify_packed(pk, host, std::move(gpu), reasons, "verify_fibsq_batch");
}


// ------------------------------------------------------- polynomial layer
std::vector<FE> evaluate_on_coset(const Poly& poly, const Coset& coset) {
    const size_t n = coset.domain_size;
    if (n == 0 || (n & (n - 1))) throw Panic("domain size must be a power of two");
    const uint32_t log_n = ceil_log2(n);
    if (coset.omega != omega(log_n)) throw Panic("coset omega must be g^((p-1)/n) (frozen spec)");
    auto gpu = Gpu::thread_default(log_n);
    auto c = to_u32(poly.coefficients);
    std::vector<uint32_t> out(n);
    gpu->check(fri_lde(gpu->ctx(), c.data(), c.size(), log_n, static_cast<uint32_t>(coset.offset.value()), out.data()),
               "fri_lde");
    return to_fe(out.data(), n);
}

namespace {
// xs == offset * w_n^i for every i (natural order, n a power of two)?
bool is_coset(const std::vector<FE>& xs, FE* offset, uint32_t* log_n) {
    const size_t n = xs.size();
    if (n == 0 || (n & (n - 1)) || xs[0] == FE::zero()) return false;
    *log_n = ceil_log2(n);
    *offset = xs[0];
    const FE w = omega(*log_n);
    FE x = xs[0];
    for (size_t i = 1; i < n; i++) {
        x = x * w;
        if (xs[i] != x) return false;
    }
    return true;
}
}  // namespace

Poly interpolate(const std::vector<FE>& xs, const std::vector<FE>& ys) {
    if (xs.size() != ys.size()) throw Panic("xs and ys must have the same length (interpolation.rs:127)");
    if (xs.empty()) return Poly();                              // Polynomial::zero() (interpolation.rs:133-136)
    FE offset;
    uint32_t log_n = 0;
    auto y = to_u32(ys);
    std::vector<uint32_t> c(xs.size());
    size_t len = 0;
    if (is_coset(xs, &offset, &log_n)) {                        // iNTT on the coset
        auto gpu = Gpu::thread_default(log_n);
        gpu->check(fri_interpolate(gpu->ctx(), y.data(), log_n, static_cast<uint32_t>(offset.value()), c.data(), &len),
                   "fri_interpolate");
    } else {
        // any other point set: the product tree from FRI_MP_INTERP_MIN points
        // (it needs next_pow2(n) <= 2^(log_n_max - 1)), O(n^2) kernels below
        auto gpu = Gpu::thread_default(ceil_log2(xs.size()) + (xs.size() >= FRI_MP_INTERP_MIN ? 1 : 0));
        auto x = to_u32(xs);
        gpu->check(fri_interpolate_points(gpu->ctx(), x.data(), y.data(), x.size(), c.data(), &len),
                   "fri_interpolate_points");
    }
    return Poly(to_fe(c.data(), len));
}

std::vector<FE> evaluate_points(const Poly& poly, const std::vector<FE>& xs) {
    const auto& cf = poly.coefficients;
    const size_t d = cf.size(), count = xs.size();
    if (count == 0) return {};
    // the tree path (min(d, count) >= FRI_MP_EVAL_MIN) needs d + next_pow2(count) - 1
    // <= 2^log_n_max and next_pow2(d) <= 2^(log_n_max - 1)
    uint32_t log_n = std::max(ceil_log2(d ? d : 1), ceil_log2(count));
    if (std::min(d, count) >= FRI_MP_EVAL_MIN)
        log_n = std::max(ceil_log2(d + ((size_t)1 << ceil_log2(count))), ceil_log2(d) + 1);
    auto gpu = Gpu::thread_default(log_n);
    const auto c = to_u32(cf), x = to_u32(xs);
    std::vector<uint32_t> out(count);
    gpu->check(fri_evaluate(gpu->ctx(), c.data(), d, x.data(), count, out.data()), "fri_evaluate");
    return to_fe(out.data(), count);
}

// ---- Poly arithmetic on the device (ops.rs:114-237) ------------------------
namespace {
std::vector<uint32_t> trimmed_u32(const std::vector<FE>& v) {
    size_t n = v.size();
    while (n > 0 && v[n - 1] == FE::zero()) n--;
    std::vector<uint32_t> o(n);
    for (size_t i = 0; i < n; i++) o[i] = static_cast<uint32_t>(v[i].value());
    return o;
}
}  // namespace

template <>
void Polynomial<P>::mul_assign(const Polynomial<P>& rhs) {
    const auto a = trimmed_u32(coefficients), b = trimmed_u32(rhs.coefficients);
    if (a.empty() || b.empty()) {                               // ops.rs:115-121
        *this = Poly();
        return;
    }
    auto gpu = Gpu::thread_default(ceil_log2(a.size() + b.size() - 1));
    std::vector<uint32_t> out(a.size() + b.size() - 1);
    size_t len = 0;
    gpu->check(fri_poly_mul(gpu->ctx(), a.data(), a.size(), b.data(), b.size(), 0, out.data(), out.size(), &len),
               "fri_poly_mul");
    *this = Poly(to_fe(out.data(), len));
}

template <>
std::pair<Poly, Poly> Polynomial<P>::div_rem(const Polynomial<P>& rhs) const {
    const auto a = trimmed_u32(coefficients), b = trimmed_u32(rhs.coefficients);
    if (b.empty()) throw Panic("Division by zero polynomial");  // ops.rs:143
    if (a.size() < b.size()) return {Poly(), Poly(to_fe(a.data(), a.size()))};   // ops.rs:145-147
    auto gpu = Gpu::thread_default(ceil_log2(a.size()) + 2);    // every la <= 2^(log_n_max - 2) is accepted
    std::vector<uint32_t> q(a.size() - b.size() + 1), r(b.size());
    size_t lq = 0, lr = 0;
    gpu->check(fri_poly_div_rem(gpu->ctx(), a.data(), a.size(), b.data(), b.size(), q.data(), q.size(), &lq, r.data(),
                                r.size(), &lr),
               "fri_poly_div_rem");
    return {Poly(to_fe(q.data(), lq)), Poly(to_fe(r.data(), lr))};
}

template <>
Poly Polynomial<P>::compose(const Polynomial<P>& other) const {
    const auto p = trimmed_u32(coefficients), q = trimmed_u32(other.coefficients);
    if (p.empty()) return Poly();
    const size_t n = q.size() <= 1 ? 1 : (p.size() - 1) * (q.size() - 1) + 1;
    const uint32_t log_n = ceil_log2(n > p.size() ? n : p.size());
    auto gpu = Gpu::thread_default(log_n);
    std::vector<uint32_t> out(n);
    size_t len = 0;
    gpu->check(fri_poly_compose(gpu->ctx(), p.data(), p.size(), q.data(), q.size(), out.data(), out.size(), &len),
               "fri_poly_compose");
    return Poly(to_fe(out.data(), len));
}

// ---- interpolation.rs:9-115 on the device ----------------------------------
template <>
Poly gen_polynomial_from_roots<P>(const std::vector<FE>& roots) {
    if (roots.empty()) return Poly::zero();                     // interpolation.rs:10-12
    auto gpu = Gpu::thread_default(ceil_log2(roots.size()));
    const auto r = to_u32(roots);
    std::vector<uint32_t> out(r.size() + 1);
    size_t len = 0;
    gpu->check(fri_poly_from_roots(gpu->ctx(), r.data(), r.size(), 0, out.data(), out.size(), &len),
               "fri_poly_from_roots");
    return Poly(to_fe(out.data(), len));
}

template <>
std::vector<Poly> gen_lagrange_polynomials<P>(const std::vector<FE>& xs) {
    const size_t n = xs.size();
    std::vector<Poly> rows;
    if (n == 0) return rows;
    auto gpu = Gpu::thread_default(ceil_log2(n));
    const auto x = to_u32(xs);
    std::vector<uint32_t> out(n * n);
    gpu->check(fri_lagrange_basis(gpu->ctx(), x.data(), n, out.data(), out.size()), "fri_lagrange_basis");
    rows.resize(n);
    for (size_t i = 0; i < n; i++) {
        // scalar_mul does not re-trim (ops.rs:194-198): n coefficients under
        // degree n - 1, also for the all-zero row of a repeated x
        rows[i].coefficients = to_fe(out.data() + i * n, n);
        rows[i].degree = static_cast<int64_t>(n) - 1;
    }
    return rows;
}

std::vector<FE> batch_inverse(const std::vector<FE>& xs) {
    if (xs.empty()) return {};
    auto gpu = Gpu::thread_default(ceil_log2(xs.size()));
    auto v = to_u32(xs);
    std::vector<uint32_t> out(v.size());
    gpu->check(fri_batch_inverse(gpu->ctx(), v.data(), out.data(), v.size()), "fri_batch_inverse");
    return to_fe(out.data(), out.size());
}

}  // namespace stark101
