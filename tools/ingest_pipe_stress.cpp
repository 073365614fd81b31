// Host-side stress test of the native ingest pipe (csrc/ingest_pipe.cpp) under
// ThreadSanitizer / AddressSanitizer, with the HIP runtime simulated on the host
// (tools/hipsim/) and fa_fold_f32 restated on the CPU (the same in-order
// left fold with separate roundings).  Many rounds on several pipes from
// several threads at once, random chunk sizes, slot counts, piece splits and
// scored / plain rows; every round is compared bit for bit with a direct CPU
// fold of the same rows.  Also: errors mid-round (a short row, mixed scores),
// a round abandoned with a chunk half filled and the pipe reused (bit-exact),
// destroy with copies possibly in flight, and finish with no rows.
// float16 pipes (the *_f16 entries) run the same way against a CPU restatement
// of fa_fold_f16: plain and scored rounds, an abandoned round then a reused
// pipe, and calls of the wrong element kind.  float64 pipes (the *_f64
// entries) likewise against a CPU restatement of fa_fold_f64, with rows handed
// over as pieces at odd byte offsets (the pack is bytewise).
//   tools/ingest_pipe_stress.sh   (builds with -fsanitize=thread, then address,undefined)
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <random>
#include <thread>
#include <vector>

#include "fedavg_hip.h"

#pragma clang fp contract(off)
#pragma GCC optimize("fp-contract=off")

static thread_local char g_msg[256] = "";
__attribute__((visibility("hidden"))) int fa_internal_fail(int code, const char* msg) {
    snprintf(g_msg, sizeof(g_msg), "%s", msg);
    return code;
}
extern "C" const char* fa_last_error(void) { return g_msg; }

// CPU restatement of fa_fold_f32 (fedavg_hip.h): acc = [acc_in +] t_0 + t_1 ...; optional divide
extern "C" int fa_fold_f32(const float* X, int64_t N, int64_t P, int64_t ldx, const float* a, const float* s,
                           const float* acc_in, float divisor, int finalize, float* out, void*) {
    for (int64_t p = 0; p < P; ++p) {
        float acc = 0.f;
        int64_t i = 0;
        if (acc_in) {
            acc = acc_in[p];
        } else if (N > 0) {
            float t = X[p] * a[0];
            if (s) t = t * s[0];
            acc = t;
            i = 1;
        }
        for (; i < N; ++i) {
            float t = X[i * ldx + p] * a[i];
            if (s) t = t * s[i];
            acc = acc + t;
        }
        out[p] = finalize ? acc / divisor : acc;
    }
    return FA_OK;
}

// ---- binary16 on the CPU --------------------------------------------------
// Exact half -> float; float -> half with round-to-nearest-even, subnormals
// kept.  A product, sum or quotient of two halves computed in float32 and
// rounded once more to half is the correctly rounded binary16 result (24 >= 2 *
// 11 + 2 bits), which is how the kernels' arithmetic is defined.
static float h2f(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1Fu, m = h & 0x3FFu;
    uint32_t u;
    if (e == 0x1Fu) {
        u = sign | 0x7F800000u | (m << 13);
    } else if (e != 0) {
        u = sign | ((e + 112u) << 23) | (m << 13);
    } else if (m == 0) {
        u = sign;
    } else {
        int sh = 0;
        uint32_t mm = m;
        while (!(mm & 0x400u)) { mm <<= 1; ++sh; }
        u = sign | ((uint32_t)(113 - sh) << 23) | ((mm & 0x3FFu) << 13);
    }
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}
static uint16_t f2h(float f) {
    uint32_t u;
    memcpy(&u, &f, sizeof u);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    const uint32_t ax = u & 0x7FFFFFFFu;
    if (ax >= 0x7F800000u) return (uint16_t)(sign | 0x7C00u | (ax > 0x7F800000u ? 0x200u : 0u));  // inf, NaN
    if (ax >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);  // >= 65520 rounds to inf
    if (ax < 0x33000000u) return sign;                          // < 2^-25 rounds to zero (2^-25 itself: tie to even)
    const int e = (int)(ax >> 23) - 127;
    uint32_t m = (ax & 0x7FFFFFu) | 0x800000u;  // 24-bit significand
    int shift = e < -14 ? 13 + (-14 - e) : 13;  // bits dropped (subnormal results drop more)
    const uint32_t keep = m >> shift, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
    uint32_t r = keep + ((rem > half || (rem == half && (keep & 1u))) ? 1u : 0u);
    if (e < -14) return (uint16_t)(sign | r);  // subnormal (r may carry into the smallest normal: same bits)
    // normal: r has the implicit bit at 0x400 (or 0x800 after a carry)
    return (uint16_t)(sign | (uint16_t)(((uint32_t)(e + 15 - 1) << 10) + r));
}
static uint16_t hmul(uint16_t x, uint16_t y) { return f2h(h2f(x) * h2f(y)); }
static uint16_t hadd(uint16_t x, uint16_t y) { return f2h(h2f(x) + h2f(y)); }
static uint16_t hdiv(uint16_t x, uint16_t y) { return f2h(h2f(x) / h2f(y)); }

// CPU restatement of fa_fold_f16 (fedavg_hip.h): binary16 products, sums and quotient in row order
extern "C" int fa_fold_f16(const uint16_t* X, int64_t N, int64_t P, int64_t ldx, const uint16_t* a,
                           const uint16_t* s, const uint16_t* acc_in, uint16_t divisor, int finalize, uint16_t* out,
                           void*) {
    if (N == 0 && !acc_in) return fa_internal_fail(FA_ERR_NO_CLIENTS, "no client results to aggregate (N == 0)");
    for (int64_t p = 0; p < P; ++p) {
        uint16_t acc = 0;
        int64_t i = 0;
        if (acc_in) {
            acc = acc_in[p];
        } else {
            acc = hmul(X[p], a[0]);
            if (s) acc = hmul(acc, s[0]);
            i = 1;
        }
        for (; i < N; ++i) {
            uint16_t t = hmul(X[i * ldx + p], a[i]);
            if (s) t = hmul(t, s[i]);
            acc = hadd(acc, t);
        }
        out[p] = finalize ? hdiv(acc, divisor) : acc;
    }
    return FA_OK;
}

// CPU restatement of fa_fold_f64 (fedavg_hip.h): binary64 products, sums and quotient in row order
extern "C" int fa_fold_f64(const double* X, int64_t N, int64_t P, int64_t ldx, const double* a, const double* s,
                           const double* acc_in, double divisor, int finalize, double* out, void*) {
    if (N == 0 && !acc_in) return fa_internal_fail(FA_ERR_NO_CLIENTS, "no client results to aggregate (N == 0)");
    for (int64_t p = 0; p < P; ++p) {
        double acc;
        int64_t i = 0;
        if (acc_in) {
            acc = acc_in[p];
        } else {
            acc = X[p] * a[0];
            if (s) acc = acc * s[0];
            i = 1;
        }
        for (; i < N; ++i) {
            double t = X[i * ldx + p] * a[i];
            if (s) t = t * s[i];
            acc = acc + t;
        }
        out[p] = finalize ? acc / divisor : acc;
    }
    return FA_OK;
}

static std::atomic<int> g_fail{0};

static void check(bool ok, const char* what) {
    if (!ok) {
        fprintf(stderr, "FAIL: %s\n", what);
        g_fail.fetch_add(1);
    }
}

static void worker(int tid, int rounds) {
    std::mt19937_64 rng(1234 + tid);
    for (int r = 0; r < rounds; ++r) {
        const int64_t P = 1 + rng() % 70000;
        const int64_t N = 1 + rng() % 40;
        const int slots = 2 + rng() % 5;
        const int64_t ldx = (P + 63) / 64 * 64;
        const int64_t chunk = ldx * 4 * (1 + rng() % 6);
        const bool scored = rng() & 1;
        std::vector<float> X(N * P), a(N), s(N);
        for (auto& v : X) v = (float)((int64_t)(rng() % 2001) - 1000) / 1024.f;
        for (int64_t i = 0; i < N; ++i) {
            a[i] = (float)(1 + rng() % 600);
            s[i] = (float)(1 + rng() % 11) / 11.f;
        }
        fa_ingest* pipe = nullptr;
        check(fa_ingest_create(&pipe, P, chunk, slots, tid % 2) == FA_OK, "create");  // two devices: the pool grows
        std::vector<float> acc(P, -1.f);
        for (int rep = 0; rep < 2; ++rep) {  // the pipe is reused
            // the announced row count: unknown, exact, too high, too low (only the chunk sizes change)
            const int64_t guess[4] = {0, N, N + 3, N > 2 ? N - 2 : 1};
            check(fa_ingest_begin(pipe, acc.data(), nullptr, guess[rng() % 4]) == FA_OK, "begin");
            for (int64_t i = 0; i < N; ++i) {
                // the row in 1-4 pieces
                std::vector<const void*> src;
                std::vector<int64_t> sz;
                int64_t off = 0;
                const int parts = 1 + rng() % 4;
                for (int k = 0; k < parts; ++k) {
                    const int64_t len = k == parts - 1 ? P - off : (P - off) * (int64_t)(rng() % 100) / 100;
                    src.push_back(X.data() + i * P + off);
                    sz.push_back(len * 4);
                    off += len;
                }
                check(fa_ingest_add(pipe, src.data(), sz.data(), (int64_t)src.size(), a[i], s[i], scored) == FA_OK,
                      "add");
            }
            float total = 0.f;
            for (int64_t i = 0; i < N; ++i) total = total + a[i];  // exact: small integers
            check(fa_ingest_finish(pipe, total) == FA_OK, "finish");
            std::vector<float> exp(P);
            fa_fold_f32(X.data(), N, P, P, a.data(), scored ? s.data() : nullptr, nullptr, total, 1, exp.data(),
                        nullptr);
            check(memcmp(exp.data(), acc.data(), P * 4) == 0, "bit-exact");
        }
        // errors mid-round, then destroy with copies possibly in flight
        check(fa_ingest_begin(pipe, acc.data(), nullptr, 0) == FA_OK, "begin 2");
        const void* src0 = X.data();
        int64_t full = P * 4, shortb = (P - 1) * 4;
        check(fa_ingest_add(pipe, &src0, &full, 1, 1.f, 1.f, 0) == FA_OK, "add ok");
        check(fa_ingest_add(pipe, &src0, &shortb, 1, 1.f, 1.f, 0) == FA_ERR_SHAPE, "short row rejected");
        check(fa_ingest_add(pipe, &src0, &full, 1, 1.f, 0.5f, 1) == FA_ERR_SHAPE, "mixed scores rejected");
        // abandon that round with a chunk half filled (the second chunk ramps to 2 rows), then
        // reuse the pipe: the abandoned rows must not join the next round
        check(fa_ingest_add(pipe, &src0, &full, 1, 7.f, 1.f, 0) == FA_OK, "add ok 2");
        check(fa_ingest_begin(pipe, acc.data(), nullptr, 0) == FA_OK, "begin after an abandoned round");
        for (int64_t i = 0; i < N; ++i) {
            const void* src = X.data() + i * P;
            check(fa_ingest_add(pipe, &src, &full, 1, a[i], s[i], 0) == FA_OK, "add after abandon");
        }
        {
            float total = 0.f;
            for (int64_t i = 0; i < N; ++i) total = total + a[i];
            check(fa_ingest_finish(pipe, total) == FA_OK, "finish after abandon");
            std::vector<float> exp(P);
            fa_fold_f32(X.data(), N, P, P, a.data(), nullptr, nullptr, total, 1, exp.data(), nullptr);
            check(memcmp(exp.data(), acc.data(), P * 4) == 0, "bit-exact after an abandoned round");
        }
        // abandoned again, now with copies possibly in flight: destroy
        check(fa_ingest_begin(pipe, acc.data(), nullptr, 0) == FA_OK, "begin 4");
        for (int k = 0; k < 3; ++k) check(fa_ingest_add(pipe, &src0, &full, 1, 1.f, 1.f, 0) == FA_OK, "add 3");
        fa_ingest_destroy(pipe);
        fa_ingest* empty = nullptr;
        check(fa_ingest_create(&empty, P, chunk, slots, 0) == FA_OK, "create 2");
        check(fa_ingest_begin(empty, acc.data(), nullptr, 5) == FA_OK, "begin 3");
        check(fa_ingest_finish(empty, 1.f) == FA_ERR_NO_CLIENTS, "empty round");
        fa_ingest_destroy(empty);
    }
}

// float16 rounds: plain and scored (pipe reused), an abandoned round then a
// clean one, wrong-kind calls on both kinds of pipe
static void worker_f16(int tid, int rounds) {
    std::mt19937_64 rng(4321 + tid);
    for (int r = 0; r < rounds; ++r) {
        const int64_t P = 1 + rng() % 70000;
        const int64_t N = 1 + rng() % 33;
        const int slots = 2 + rng() % 5;
        const int64_t ldx = (P + 63) / 64 * 64;
        const int64_t chunk = ldx * 2 * (1 + rng() % 6);
        std::vector<uint16_t> X(N * P), a(N), s(N);
        for (auto& v : X) v = f2h((float)((int64_t)(rng() % 2001) - 1000) / 1024.f);
        float totalf = 0.f;
        for (int64_t i = 0; i < N; ++i) {
            const float w = (float)(1 + rng() % 40);
            totalf += w;  // <= 1320: exact in binary16's integer range up to 2048
            a[i] = f2h(w);
            s[i] = f2h((float)(1 + rng() % 11) / 11.f);
        }
        const uint16_t total = f2h(totalf);
        fa_ingest* pipe = nullptr;
        check(fa_ingest_create_f16(&pipe, P, chunk, slots, tid % 2) == FA_OK, "create f16");
        check(fa_ingest_rows_per_chunk(pipe) == (int)(chunk / (ldx * 2)), "rows per chunk f16");
        std::vector<uint16_t> acc(P, 0x7E00u), exp(P);
        for (int rep = 0; rep < 2; ++rep) {  // plain, then scored, on the same pipe
            const bool scored = rep == 1;
            const int64_t guess[4] = {0, N, N + 3, N > 2 ? N - 2 : 1};
            check(fa_ingest_begin_f16(pipe, acc.data(), nullptr, guess[rng() % 4]) == FA_OK, "begin f16");
            for (int64_t i = 0; i < N; ++i) {
                // the row in 1-4 pieces of any whole number of halves (odd counts included)
                std::vector<const void*> src;
                std::vector<int64_t> sz;
                int64_t off = 0;
                const int parts = 1 + rng() % 4;
                for (int k = 0; k < parts; ++k) {
                    const int64_t len = k == parts - 1 ? P - off : (P - off) * (int64_t)(rng() % 100) / 100;
                    src.push_back(X.data() + i * P + off);
                    sz.push_back(len * 2);
                    off += len;
                }
                check(fa_ingest_add_f16(pipe, src.data(), sz.data(), (int64_t)src.size(), a[i], s[i], scored) == FA_OK,
                      "add f16");
            }
            check(fa_ingest_finish_f16(pipe, total) == FA_OK, "finish f16");
            fa_fold_f16(X.data(), N, P, P, a.data(), scored ? s.data() : nullptr, nullptr, total, 1, exp.data(),
                        nullptr);
            check(memcmp(exp.data(), acc.data(), P * 2) == 0, "bit-exact f16");
        }
        // wrong-kind calls: refused, and the pipe is left as it was
        const void* src0 = X.data();
        int64_t full = P * 2, shortb = (P - 1) * 2;
        std::vector<float> acc32(P);
        check(fa_ingest_begin(pipe, acc32.data(), nullptr, 0) == FA_ERR_ARG, "f32 begin on an f16 pipe");
        check(fa_ingest_begin_f16(pipe, acc.data(), nullptr, 0) == FA_OK, "begin f16 2");
        check(fa_ingest_add(pipe, &src0, &full, 1, 1.f, 1.f, 0) == FA_ERR_ARG, "f32 add on an f16 pipe");
        check(fa_ingest_finish(pipe, 1.f) == FA_ERR_ARG, "f32 finish on an f16 pipe");
        // errors mid-round, a chunk half filled, then the pipe reused: the abandoned rows do not join
        check(fa_ingest_add_f16(pipe, &src0, &full, 1, 0x3C00, 0x3C00, 0) == FA_OK, "add f16 ok");
        check(fa_ingest_add_f16(pipe, &src0, &shortb, 1, 0x3C00, 0x3C00, 0) == FA_ERR_SHAPE, "short f16 row rejected");
        check(fa_ingest_add_f16(pipe, &src0, &full, 1, 0x3C00, 0x3800, 1) == FA_ERR_SHAPE, "mixed scores rejected f16");
        check(fa_ingest_add_f16(pipe, &src0, &full, 1, 0x4700, 0x3C00, 0) == FA_OK, "add f16 ok 2");
        check(fa_ingest_begin_f16(pipe, acc.data(), nullptr, 0) == FA_OK, "begin f16 after an abandoned round");
        for (int64_t i = 0; i < N; ++i) {
            const void* src = X.data() + i * P;
            check(fa_ingest_add_f16(pipe, &src, &full, 1, a[i], s[i], 0) == FA_OK, "add f16 after abandon");
        }
        check(fa_ingest_finish_f16(pipe, total) == FA_OK, "finish f16 after abandon");
        fa_fold_f16(X.data(), N, P, P, a.data(), nullptr, nullptr, total, 1, exp.data(), nullptr);
        check(memcmp(exp.data(), acc.data(), P * 2) == 0, "bit-exact f16 after an abandoned round");
        fa_ingest_destroy(pipe);
        // the reverse: f16 entries on a float32 pipe
        fa_ingest* p32 = nullptr;
        check(fa_ingest_create(&p32, P, chunk * 2, slots, 0) == FA_OK, "create f32");
        check(fa_ingest_begin_f16(p32, acc.data(), nullptr, 0) == FA_ERR_ARG, "f16 begin on an f32 pipe");
        check(fa_ingest_begin(p32, acc32.data(), nullptr, 0) == FA_OK, "begin f32");
        check(fa_ingest_add_f16(p32, &src0, &full, 1, 0x3C00, 0x3C00, 0) == FA_ERR_ARG, "f16 add on an f32 pipe");
        check(fa_ingest_finish_f16(p32, 0x3C00) == FA_ERR_ARG, "f16 finish on an f32 pipe");
        check(fa_ingest_finish(p32, 1.f) == FA_ERR_NO_CLIENTS, "empty f32 round after refused calls");
        fa_ingest_destroy(p32);
    }
}

// float64 rounds: plain and scored (pipe reused), an abandoned round then a
// clean one, wrong-kind calls on every pair of kinds.  The rows live in a byte
// buffer at an odd offset, as views into an NPZ blob do.
static void worker_f64(int tid, int rounds) {
    std::mt19937_64 rng(8642 + tid);
    for (int r = 0; r < rounds; ++r) {
        const int64_t P = 1 + rng() % 40000;
        const int64_t N = 1 + rng() % 33;
        const int slots = 2 + rng() % 5;
        const int64_t ldx = (P + 63) / 64 * 64;
        const int64_t chunk = ldx * 8 * (1 + rng() % 6);
        std::vector<double> X(N * P), a(N), s(N);
        for (auto& v : X) v = (double)((int64_t)(rng() % 2000001) - 1000000) / 3.0;  // low mantissa bits filled
        double total = 0.0;
        for (int64_t i = 0; i < N; ++i) {
            a[i] = (double)(1 + rng() % 600);
            total += a[i];
            s[i] = (double)(1 + rng() % 11) / 11.0;
        }
        const int64_t shift = 1 + rng() % 7;  // the rows' byte offset inside the blob: never 8-B aligned
        std::vector<uint8_t> blob((size_t)(N * P * 8 + 8));
        memcpy(blob.data() + shift, X.data(), (size_t)(N * P * 8));
        fa_ingest* pipe = nullptr;
        check(fa_ingest_create_f64(&pipe, P, chunk, slots, tid % 2) == FA_OK, "create f64");
        check(fa_ingest_rows_per_chunk(pipe) == (int)(chunk / (ldx * 8)), "rows per chunk f64");
        std::vector<double> acc(P, -1.0), exp(P);
        for (int rep = 0; rep < 2; ++rep) {  // plain, then scored, on the same pipe
            const bool scored = rep == 1;
            const int64_t guess[4] = {0, N, N + 3, N > 2 ? N - 2 : 1};
            check(fa_ingest_begin_f64(pipe, acc.data(), nullptr, guess[rng() % 4]) == FA_OK, "begin f64");
            for (int64_t i = 0; i < N; ++i) {
                // the row in 1-4 pieces of any number of bytes (a double may straddle two pieces)
                std::vector<const void*> src;
                std::vector<int64_t> sz;
                int64_t off = 0;
                const int parts = 1 + rng() % 4;
                for (int k = 0; k < parts; ++k) {
                    const int64_t len = k == parts - 1 ? P * 8 - off : (P * 8 - off) * (int64_t)(rng() % 100) / 100;
                    src.push_back(blob.data() + shift + i * P * 8 + off);
                    sz.push_back(len);
                    off += len;
                }
                check(fa_ingest_add_f64(pipe, src.data(), sz.data(), (int64_t)src.size(), a[i], s[i], scored) == FA_OK,
                      "add f64");
            }
            check(fa_ingest_finish_f64(pipe, total) == FA_OK, "finish f64");
            fa_fold_f64(X.data(), N, P, P, a.data(), scored ? s.data() : nullptr, nullptr, total, 1, exp.data(),
                        nullptr);
            check(memcmp(exp.data(), acc.data(), P * 8) == 0, "bit-exact f64");
        }
        // wrong-kind calls: refused, and the pipe is left as it was
        const void* src0 = blob.data() + shift;
        int64_t full = P * 8, shortb = (P - 1) * 8;
        std::vector<float> acc32(P);
        std::vector<uint16_t> acc16(P);
        check(fa_ingest_begin(pipe, acc32.data(), nullptr, 0) == FA_ERR_ARG, "f32 begin on an f64 pipe");
        check(fa_ingest_begin_f16(pipe, acc16.data(), nullptr, 0) == FA_ERR_ARG, "f16 begin on an f64 pipe");
        check(fa_ingest_begin_f64(pipe, acc.data(), nullptr, 0) == FA_OK, "begin f64 2");
        check(fa_ingest_add(pipe, &src0, &full, 1, 1.f, 1.f, 0) == FA_ERR_ARG, "f32 add on an f64 pipe");
        check(fa_ingest_add_f16(pipe, &src0, &full, 1, 0x3C00, 0x3C00, 0) == FA_ERR_ARG, "f16 add on an f64 pipe");
        check(fa_ingest_finish(pipe, 1.f) == FA_ERR_ARG, "f32 finish on an f64 pipe");
        check(fa_ingest_finish_f16(pipe, 0x3C00) == FA_ERR_ARG, "f16 finish on an f64 pipe");
        // errors mid-round, a chunk half filled, then the pipe reused: the abandoned rows do not join
        check(fa_ingest_add_f64(pipe, &src0, &full, 1, 1.0, 1.0, 0) == FA_OK, "add f64 ok");
        check(fa_ingest_add_f64(pipe, &src0, &shortb, 1, 1.0, 1.0, 0) == FA_ERR_SHAPE, "short f64 row rejected");
        check(fa_ingest_add_f64(pipe, &src0, &full, 1, 1.0, 0.5, 1) == FA_ERR_SHAPE, "mixed scores rejected f64");
        check(fa_ingest_add_f64(pipe, &src0, &full, 1, 7.0, 1.0, 0) == FA_OK, "add f64 ok 2");
        check(fa_ingest_begin_f64(pipe, acc.data(), nullptr, 0) == FA_OK, "begin f64 after an abandoned round");
        for (int64_t i = 0; i < N; ++i) {
            const void* src = blob.data() + shift + i * P * 8;
            check(fa_ingest_add_f64(pipe, &src, &full, 1, a[i], s[i], 0) == FA_OK, "add f64 after abandon");
        }
        check(fa_ingest_finish_f64(pipe, total) == FA_OK, "finish f64 after abandon");
        fa_fold_f64(X.data(), N, P, P, a.data(), nullptr, nullptr, total, 1, exp.data(), nullptr);
        check(memcmp(exp.data(), acc.data(), P * 8) == 0, "bit-exact f64 after an abandoned round");
        fa_ingest_destroy(pipe);
        // the reverse: f64 entries on a float32 and on a float16 pipe
        fa_ingest* other[2] = {nullptr, nullptr};
        check(fa_ingest_create(&other[0], P, chunk, slots, 0) == FA_OK, "create f32");
        check(fa_ingest_create_f16(&other[1], P, chunk, slots, 0) == FA_OK, "create f16");
        for (fa_ingest* q : other) {
            check(fa_ingest_begin_f64(q, acc.data(), nullptr, 0) == FA_ERR_ARG, "f64 begin on another pipe");
            check(fa_ingest_add_f64(q, &src0, &full, 1, 1.0, 1.0, 0) == FA_ERR_ARG, "f64 add on another pipe");
            check(fa_ingest_finish_f64(q, 1.0) == FA_ERR_ARG, "f64 finish on another pipe");
        }
        check(fa_ingest_begin(other[0], acc32.data(), nullptr, 0) == FA_OK, "begin f32 after refused calls");
        check(fa_ingest_finish(other[0], 1.f) == FA_ERR_NO_CLIENTS, "empty f32 round after refused calls");
        fa_ingest_destroy(other[0]);
        fa_ingest_destroy(other[1]);
    }
}

// f2h / h2f against a few known patterns (the restated fold rests on them)
static void check_half() {
    check(f2h(1.0f) == 0x3C00 && f2h(-2.0f) == 0xC000 && f2h(65504.f) == 0x7BFF, "f2h normals");
    check(f2h(65519.99f) == 0x7BFF && f2h(65520.f) == 0x7C00, "f2h overflow threshold");
    check(f2h(5.9604645e-8f) == 0x0001 && f2h(2.9802322e-8f) == 0x0000 && f2h(2.98024e-8f) == 0x0001, "f2h subnormal");
    check(f2h(6.097555e-5f) == 0x03FF && f2h(6.1035156e-5f) == 0x0400, "f2h subnormal / normal border");
    check(f2h(1.00048828125f) == 0x3C00 && f2h(1.00146484375f) == 0x3C02, "f2h ties to even");
    check(f2h(-0.0f) == 0x8000, "f2h -0");
    for (uint32_t h = 0; h < 0x10000u; ++h) {
        const uint16_t b = f2h(h2f((uint16_t)h));
        const bool nan = (h & 0x7C00u) == 0x7C00u && (h & 0x3FFu);
        check(nan ? ((b & 0x7C00u) == 0x7C00u && (b & 0x3FFu)) : b == h, "half round trip");
    }
}

int main() {
    check_half();
    std::vector<std::thread> ts;
    for (int t = 0; t < 3; ++t) ts.emplace_back(worker, t, 12);
    for (int t = 0; t < 2; ++t) ts.emplace_back(worker_f16, t, 8);
    for (int t = 0; t < 2; ++t) ts.emplace_back(worker_f64, t, 8);
    for (auto& t : ts) t.join();
    if (g_fail.load()) {
        fprintf(stderr, "%d failures\n", g_fail.load());
        return 1;
    }
    printf("ingest_pipe_stress: ok\n");
    return 0;
}
