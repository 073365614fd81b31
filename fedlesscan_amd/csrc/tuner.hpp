// tuner.hpp -- measured kernel-form choice for the fold entries of
// libfedavg_hip.so (host code only: the HIP runtime API, no kernels, so the
// state machine also builds against tools/tunersim for a host stress test,
// tools/tuner_stress.cpp).  Used by fold_kernels.hpp.
#pragma once

#include <hip/hip_runtime_api.h>
#include <fcntl.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

// internal linkage (the libraries export exactly their headers' symbols)
namespace {
namespace fa_tune {

constexpr int kTuneOk = 0;  // FA_OK: launch() returns an FA status

// ---------------------------------------------------------------------------
// Measured form choice (the tuner).  The shape policy's picks
// (fold_kernels.hpp pick_f32 / pick_bf16) are fitted to sweeps over measured
// shapes; between those shapes every form swings with how the tiles fall on
// the CUs (1024 x 909K params: the policy's form 0.70 ms, the even split
// 0.53 ms; 256 x 3.57M bf16: 0.337 against 0.295 ms; profiles/r03_slot_sweep/).
// Every form computes the same bits, and a plain one-shot fold overwrites its
// whole output, so the FIRST call of a new shape runs every candidate form on
// the caller's own data, on the caller's stream: one untimed launch of each
// (code-object load, cold TLBs, clocks up from idle), then two timed passes in
// opposite orders, `batch` back-to-back launches of a form between two events
// (batch sized to ~0.3 ms, so launch gaps do not decide between forms of a
// 20 us kernel: timing single launches between events misranked them,
// profiles/r03_tuner/probe_single_launch.log); a form's time is its faster
// pass.  Whichever form ran last, the output is the fold.  Nothing
// synchronises: later calls read the events with hipEventQuery and run the
// policy's pick until they are complete; from then on the shape runs the
// fastest form -- the policy's own pick unless another beats it by more than
// 3 % (box-to-box spread is ~2-5 %).
//
// A shape is (device, kind, client-count bucket, policy form, P, pitch,
// scored).  The client count enters as its power-of-two bucket (round 4): in
// FL the number of results per round moves with stragglers and failures, and
// the forms' ranking follows the column tiling, not the exact row count, so a
// round with 1000 clients reuses the decision measured at 1024 (the policy
// form is part of the key, so a bucket never spans two policy picks).
//
// Decisions persist across processes (round 4): the reference builds a fresh
// strategy per FaaS invocation (aggregation.py:71-75) under a 60 s OpenWhisk
// limit (deploy.sh:9-10), and every cold process used to re-pay the sweep.
// A text cache file -- one line per decided shape, keyed by the device's
// identity (gfx arch and CU count) and the library's ABI version, forms by
// NAME -- is read on the first tuned call and rewritten under an exclusive
// flock(2) through a temp file + rename(2) after each new decision, merged
// with what other processes wrote meanwhile.  Lines that do not parse, carry
// another ABI or name an unknown form are ignored, so a stale or corrupt
// file only costs a re-measurement.  FEDAVG_TUNE_CACHE=<path> moves it, =0
// (or fa_tune_cache_path("")) turns it off; default
// $XDG_CACHE_HOME/fedlesscan_amd/tuner.txt or ~/.cache/fedlesscan_amd/tuner.txt.
// The same lines move decisions between processes (fa_tune_export /
// fa_tune_import: a multi-GPU job runs rank 0's forms on every rank).
//
// Step-form decisions (round 5): at N > 1 ShardedAggregator runs an exchange
// step either as one fold launch per step or one launch per round; "auto"
// keeps the choice a probe measured on this machine.  Those choices live in
// the same file as "fedavg-step" lines (key: device identity, dtype, world
// size, client bucket, P, the layout's slot widths), so a cold process -- one
// FaaS invocation -- runs the measured step form without probing, and
// export/import carry them with the kernel forms.
//
// File I/O never runs under the tuner's mutex: a decision queues its line,
// and the call that made it merges the queue into the file after releasing
// the mutex, taking the file lock with LOCK_NB and a bounded retry (a file
// held elsewhere or a slow filesystem delays the write to a later call, never
// a fold).
//
// FEDAVG_AUTOTUNE=0 (or fa_set_autotune(0)) keeps the policy pick;
// FEDAVG_AUTOTUNE_LOG=1 prints every decision with each candidate's time.
// ---------------------------------------------------------------------------
constexpr float kTuneMargin = 0.97f;
constexpr double kTuneBatchMs = 0.3;  // timed span per candidate
constexpr int kTuneMaxBatch = 32;
constexpr const char* kCacheMagic = "fedavg-tune";
constexpr const char* kStepMagic = "fedavg-step";
constexpr int kCacheFormat = 1;
constexpr size_t kCacheMaxLines = 4096;

// power-of-two bucket of a client count (1, 2, 4, ..., the next >= N)
inline int64_t n_bucket(int64_t N) {
    int64_t b = 1;
    while (b < N && b < ((int64_t)1 << 62)) b <<= 1;
    return b;
}

class Tuner {
  public:
    // names a (kind, form) pair; resolves a name back (-1: unknown); the
    // identity of a device for the cache ("gfx950:256"; "" = do not persist)
    typedef const char* (*FormName)(int kind, int form);
    typedef int (*FormFromName)(int kind, const char* name);
    typedef std::string (*DeviceIdent)(int dev);
    explicit Tuner(FormName name = nullptr, FormFromName from_name = nullptr, DeviceIdent ident = nullptr,
                   int abi = 0)
        : name_(name), from_name_(from_name), ident_(ident), abi_(abi) {}
    ~Tuner() { flush_persist(); }  // best effort, bounded (flush_persist)
    Tuner(const Tuner&) = delete;
    Tuner& operator=(const Tuner&) = delete;
    static int env_mode() {
        const char* e = getenv("FEDAVG_AUTOTUNE");
        return (e && e[0] == '0') ? 0 : 1;
    }
    int set_mode(int m) {
        const int prev = mode_.load();
        if (m >= 0) mode_.store(m ? 1 : 0);
        return prev;
    }
    // The cache file ("" = none).  Takes effect for devices not yet loaded;
    // decisions already made stay in memory.
    void set_cache_path(const std::string& p) {
        std::lock_guard<std::mutex> lk(mu_);
        path_ = p;
        path_set_ = true;
        loaded_.clear();
        steps_loaded_ = false;
    }
    std::string cache_path() {
        std::lock_guard<std::mutex> lk(mu_);
        return path_locked();
    }
    // Run this call's fold: launch(form) enqueues one fold of that form and
    // returns an FA status.  `cands(v)` fills the candidate forms (v[0] = the
    // policy pick) the first time the shape is seen; a single candidate means
    // the shape is not measured; `bytes` sizes the batch.  Runs on the
    // stream's device (the callers hold a StreamDevice).
    template <class Cands, class Launch>
    int run(int kind, int64_t N, int64_t P, int64_t ldx, bool scored, int policy, double bytes, hipStream_t st,
            Cands cands, Launch launch) {
        if (!mode_.load()) return launch(policy);
        Flush flush_after{this};  // destroyed after every lock_guard below: merges queued lines unlocked
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) {
            (void)hipGetLastError();
            return launch(policy);
        }
        const Key key{dev, kind, n_bucket(N), policy, P, ldx, scored ? 1 : 0};
        // no event calls inside a graph capture: neither the measurement nor
        // the queries of an earlier one (hipEventQuery is not capture-safe)
        auto capturing = [&] {
            hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
            if (hipStreamIsCapturing(st, &cs) != hipSuccess) {
                (void)hipGetLastError();
                return true;  // unknown: treat as capturing
            }
            return cs != hipStreamCaptureStatusNone;
        };
        Entry* e = nullptr;
        bool explore = false;
        {
            std::lock_guard<std::mutex> lk(mu_);
            auto it = map_.find(key);
            if (it == map_.end()) {
                if (capturing()) return launch(policy);
                Entry fresh;
                cands(fresh.cand);
                fresh.key = key;
                fresh.N = N;
                if (fresh.cand.size() <= 1) fresh.chosen = policy;
                if (fresh.chosen < 0) {  // a decision from the cache file or another process
                    load_locked(dev);
                    auto pr = preset_.find(disk_key(key));
                    if (pr != preset_.end()) fresh.chosen = pr->second;
                }
                it = map_.emplace(key, std::move(fresh)).first;
                explore = it->second.chosen < 0;
            }
            e = &it->second;  // std::map nodes are stable
            if (!explore) {
                if (e->chosen < 0) {
                    if (capturing()) return launch(e->cand[0]);
                    harvest(*e);
                    if (e->chosen < 0) return launch(e->cand[0]);  // measurement still in flight
                }
                return launch(e->chosen);
            }
        }
        // First call of the shape: time every candidate (this thread owns the
        // entry's events until `armed` is set; other threads run the policy).
        const double est_ms = bytes / 5.0e9;  // ~5 TB/s
        int batch = (int)(kTuneBatchMs / (est_ms > 1e-6 ? est_ms : 1e-6)) + 1;
        if (batch > kTuneMaxBatch) batch = kTuneMaxBatch;
        const int n = (int)e->cand.size();
        std::vector<hipEvent_t> ev(4 * (size_t)n, nullptr);  // [pass][candidate][start, end]
        bool timed = true;
        for (auto& x : ev)
            if (hipEventCreate(&x) != hipSuccess) {
                (void)hipGetLastError();
                x = nullptr;
                timed = false;
            }
        int rc = kTuneOk;
        // untimed: one launch of every form (code-object loads, cold TLBs; the
        // clocks come up from idle), then two timed passes in opposite orders,
        // so a drift over the measurement favours no candidate
        for (int c = 0; c < n && rc == kTuneOk; ++c) rc = launch(e->cand[c]);
        for (int pass = 0; pass < 2; ++pass)
            for (int j = 0; j < n && rc == kTuneOk; ++j) {
                const int c = pass == 0 ? j : n - 1 - j;
                hipEvent_t* pe = &ev[2 * ((size_t)pass * n + c)];
                if (timed && hipEventRecord(pe[0], st) != hipSuccess) timed = false;
                for (int b = 0; b < batch && rc == kTuneOk; ++b) rc = launch(e->cand[c]);
                if (timed && hipEventRecord(pe[1], st) != hipSuccess) timed = false;
            }
        if (!timed) (void)hipGetLastError();
        std::lock_guard<std::mutex> lk(mu_);
        e->batch = batch;
        e->events = ev;
        if (rc != kTuneOk || !timed) e->chosen = e->cand[0];  // a failed or untimed measurement keeps the policy
        e->armed = true;
        if (e->chosen >= 0) release(*e);
        return rc;
    }
    int pending() {
        Flush flush_after{this};
        std::lock_guard<std::mutex> lk(mu_);
        int n = 0;
        for (auto& kv : map_) {
            if (kv.second.chosen >= 0) continue;
            harvest(kv.second);  // the shape may have all it needs without a further call
            if (kv.second.chosen < 0) ++n;
        }
        return n;
    }
    // chosen form (>= 0), -1 while the shape is being measured, -2 unknown shape
    int chosen(int dev, int kind, int64_t N, int policy, int64_t P, int64_t ldx, bool scored) {
        Flush flush_after{this};
        std::lock_guard<std::mutex> lk(mu_);
        auto it = map_.find(Key{dev, kind, n_bucket(N), policy, P, ldx, scored ? 1 : 0});
        if (it == map_.end()) return -2;
        if (it->second.chosen < 0) harvest(it->second);
        return it->second.chosen;
    }
    // Every decided shape of this process, as cache-file lines.
    std::string export_text() {
        std::lock_guard<std::mutex> lk(mu_);
        std::string out;
        for (auto& kv : map_) {
            if (kv.second.chosen < 0) continue;
            const std::string id = ident_of(std::get<0>(kv.first));
            if (!id.empty()) out += line_of(id, kv.first, kv.second.chosen);
        }
        for (auto& kv : steps_) out += step_line(kv.first, kv.second);
        return out;
    }
    // Apply decisions given as cache-file lines (every device whose identity
    // matches a line takes it, now and for shapes it has not seen yet).
    // Returns the number of lines applied.
    int import_text(const std::string& text) {
        std::lock_guard<std::mutex> lk(mu_);
        int applied = 0;
        size_t pos = 0;
        while (pos < text.size()) {
            size_t nl = text.find('\n', pos);
            if (nl == std::string::npos) nl = text.size();
            DiskKey dk;
            int form = -1;
            std::string sk;
            int one = -1;
            if (parse_step_line(text.substr(pos, nl - pos), sk, one)) {
                steps_[sk] = one;
                ++applied;
            } else if (parse_line(text.substr(pos, nl - pos), dk, form)) {
                preset_[dk] = form;
                for (auto& kv : map_) {
                    if (disk_key(kv.first) != dk) continue;
                    // a measurement in flight is dropped: its events now (armed), or by the
                    // thread still issuing it, which releases them when it sees a decision
                    if (kv.second.armed) release(kv.second);
                    kv.second.chosen = form;
                }
                ++applied;
            }
            pos = nl + 1;
        }
        return applied;
    }

    // ---- step-form decisions ------------------------------------------------
    // key: "<ident> <dtype> <world> <client bucket> <P> <w0,w1,...>" (the
    // caller's device identity, "f32" or "bf16" -- "f32.peer" / "bf16.peer"
    // for steps whose exchange is the peer copy, "float16", "float64" -- the slot widths of its
    // layout).  lookup: 1 one launch, 0 per-round launches, -1 no decision
    // (the file is read on the first lookup; -2: a malformed key).
    int step_lookup(const std::string& key) {
        std::string k;
        if (!canon_step_key(key, k)) return -2;
        std::lock_guard<std::mutex> lk(mu_);
        load_steps_locked();
        auto it = steps_.find(k);
        return it == steps_.end() ? -1 : it->second;
    }
    // Record a decision (this process, and queued for the file).  false: a
    // malformed key.
    bool step_record(const std::string& key, bool one_launch) {
        std::string k;
        if (!canon_step_key(key, k)) return false;
        {
            std::lock_guard<std::mutex> lk(mu_);
            load_steps_locked();
            steps_[k] = one_launch ? 1 : 0;
            queue_.push_back(step_line(k, one_launch ? 1 : 0));
            queued_.store(true);
        }
        flush_persist();
        return true;
    }

  private:
    struct Flush {
        Tuner* t;
        ~Flush() { t->flush_persist(); }
    };
    // (dev, kind, client bucket, policy form, P, ldx, scored)
    typedef std::tuple<int, int, int64_t, int, int64_t, int64_t, int> Key;
    // (device identity, kind, client bucket, policy NAME, P, ldx, scored)
    typedef std::tuple<std::string, int, int64_t, std::string, int64_t, int64_t, int> DiskKey;
    struct Entry {
        std::vector<int> cand;
        std::vector<hipEvent_t> events;  // [2(pass*n + c)] start, [... + 1] end of candidate c's batch
        int batch = 1, chosen = -1;
        bool armed = false;  // the exploring call has recorded every event
        Key key;
        int64_t N = 0;       // the client count measured (the log)
    };
    void release(Entry& e) {
        for (hipEvent_t x : e.events)
            if (x) (void)hipEventDestroy(x);
        e.events.clear();
    }
    // ---- the cache file -------------------------------------------------------
    std::string ident_of(int dev) {
        auto it = ident_cache_.find(dev);
        if (it != ident_cache_.end()) return it->second;
        std::string id = ident_ ? ident_(dev) : std::string();
        for (char& c : id)
            if (c == ' ' || c == '\n' || c == '\t') c = '_';
        ident_cache_[dev] = id;
        return id;
    }
    DiskKey disk_key(const Key& k) {
        return DiskKey{ident_of(std::get<0>(k)), std::get<1>(k), std::get<2>(k),
                       form_name(std::get<1>(k), std::get<3>(k)), std::get<4>(k), std::get<5>(k), std::get<6>(k)};
    }
    std::string line_of(const std::string& id, const Key& k, int form) {
        char buf[512];
        snprintf(buf, sizeof(buf), "%s %d %s %d %d %lld %s %lld %lld %d %s\n", kCacheMagic, kCacheFormat, id.c_str(),
                 abi_, std::get<1>(k), (long long)std::get<2>(k), form_name(std::get<1>(k), std::get<3>(k)),
                 (long long)std::get<4>(k), (long long)std::get<5>(k), std::get<6>(k),
                 form_name(std::get<1>(k), form));
        return buf;
    }
    // One cache line -> key + form, or false (malformed, other format or ABI,
    // a form this library does not know).
    bool parse_line(const std::string& line, DiskKey& dk, int& form) const {
        char magic[32], id[128], pol[96], fname[96];
        int fmt = 0, abi = 0, kind = 0, scored = 0;
        long long nb = 0, P = 0, ldx = 0;
        char tail = 0;
        if (line.size() > 400) return false;
        const int got = sscanf(line.c_str(), "%31s %d %127s %d %d %lld %95s %lld %lld %d %95s %c", magic, &fmt, id,
                               &abi, &kind, &nb, pol, &P, &ldx, &scored, fname, &tail);
        if (got != 11 || strcmp(magic, kCacheMagic) != 0 || fmt != kCacheFormat || abi != abi_) return false;
        if (kind < 1 || kind > 16 || nb < 1 || (nb & (nb - 1)) || P < 1 || ldx < P || (scored != 0 && scored != 1))
            return false;
        if (!from_name_ || from_name_(kind, pol) < 0) return false;
        form = from_name_(kind, fname);
        if (form < 0) return false;
        dk = DiskKey{std::string(id), kind, (int64_t)nb, std::string(pol), (int64_t)P, (int64_t)ldx, scored};
        return true;
    }
    std::string path_locked() {
        if (!path_set_) {
            path_set_ = true;
            const char* e = getenv("FEDAVG_TUNE_CACHE");
            if (e) {
                path_ = (e[0] == '0' && e[1] == 0) ? std::string() : std::string(e);
            } else {
                const char* x = getenv("XDG_CACHE_HOME");
                const char* h = getenv("HOME");
                if (x && x[0]) path_ = std::string(x) + "/fedlesscan_amd/tuner.txt";
                else if (h && h[0]) path_ = std::string(h) + "/.cache/fedlesscan_amd/tuner.txt";
            }
        }
        return path_;
    }
    static std::string read_file(const std::string& p) {
        std::string s;
        FILE* f = fopen(p.c_str(), "rb");
        if (!f) return s;
        char buf[65536];
        size_t k;
        while ((k = fread(buf, 1, sizeof(buf), f)) > 0 && s.size() < ((size_t)8 << 20)) s.append(buf, k);
        fclose(f);
        return s;
    }
    // Under mu_: read the file's decisions for this device's identity once.
    void load_locked(int dev) {
        const std::string id = ident_of(dev);
        if (id.empty() || loaded_.count(id)) return;
        loaded_[id] = true;
        const std::string p = path_locked();
        if (p.empty()) return;
        const std::string text = read_file(p);
        size_t pos = 0;
        while (pos < text.size()) {
            size_t nl = text.find('\n', pos);
            if (nl == std::string::npos) nl = text.size();
            DiskKey dk;
            int form = -1;
            if (parse_line(text.substr(pos, nl - pos), dk, form) && std::get<0>(dk) == id) preset_[dk] = form;
            pos = nl + 1;
        }
    }
    static void make_dirs(const std::string& p) {
        for (size_t i = 1; i < p.size(); ++i)
            if (p[i] == '/') (void)mkdir(p.substr(0, i).c_str(), 0755);
    }
    // ---- step lines --------------------------------------------------------
    // "<ident> <dtype> <world> <bucket> <P> <widths>" -> the same fields
    // re-printed (canonical), or false
    static bool canon_step_key(const std::string& key, std::string& out) {
        char id[128], dt[16], widths[400];
        long long world = 0, nb = 0, P = 0;
        char tail = 0;
        if (key.size() > 500) return false;
        if (sscanf(key.c_str(), "%127s %15s %lld %lld %lld %399s %c", id, dt, &world, &nb, &P, widths, &tail) != 6)
            return false;
        // "float16" / "float64": the float16 and float64 steps (RCCL exchange only; the short "f16" and
        // "f64" stay malformed, as before them)
        if ((strcmp(dt, "f32") != 0 && strcmp(dt, "bf16") != 0 && strcmp(dt, "f32.peer") != 0 &&
             strcmp(dt, "bf16.peer") != 0 && strcmp(dt, "float16") != 0 && strcmp(dt, "float64") != 0) ||
            world < 1 || world > 4096 || nb < 1 || (nb & (nb - 1)) || P < 1)
            return false;
        // widths: 1..8 positive integers separated by commas
        int n = 0;
        const char* q = widths;
        while (*q) {
            if (*q < '0' || *q > '9') return false;
            char* end = nullptr;
            const long long w = strtoll(q, &end, 10);
            if (w < 1 || ++n > 8) return false;
            q = end;
            if (*q == ',') {
                ++q;
                if (!*q) return false;
            } else if (*q) {
                return false;
            }
        }
        if (n < 1) return false;
        char buf[600];
        snprintf(buf, sizeof(buf), "%s %s %lld %lld %lld %s", id, dt, world, nb, P, widths);
        out = buf;
        return true;
    }
    std::string step_line(const std::string& k, int one) const {
        char buf[700];
        snprintf(buf, sizeof(buf), "%s %d %d %s %s\n", kStepMagic, kCacheFormat, abi_, k.c_str(),
                 one ? "one" : "per");
        return buf;
    }
    // "fedavg-step <format> <abi> <key...> one|per" -> canonical key + choice
    bool parse_step_line(const std::string& line, std::string& key, int& one) const {
        char magic[32], rest[600], choice[8];
        int fmt = 0, abi = 0, used = 0;
        if (line.size() > 600) return false;
        if (sscanf(line.c_str(), "%31s %d %d %n", magic, &fmt, &abi, &used) != 3 || strcmp(magic, kStepMagic) != 0 ||
            fmt != kCacheFormat || abi != abi_)
            return false;
        std::string body = line.substr((size_t)used);
        while (!body.empty() && (body.back() == ' ' || body.back() == '\r')) body.pop_back();
        const size_t sp = body.rfind(' ');
        if (sp == std::string::npos) return false;
        snprintf(choice, sizeof(choice), "%s", body.substr(sp + 1).c_str());
        if (strcmp(choice, "one") == 0) one = 1;
        else if (strcmp(choice, "per") == 0) one = 0;
        else return false;
        snprintf(rest, sizeof(rest), "%s", body.substr(0, sp).c_str());
        return canon_step_key(rest, key);
    }
    // Under mu_: read the file's step lines once (every identity: the key holds it).
    void load_steps_locked() {
        if (steps_loaded_) return;
        steps_loaded_ = true;
        const std::string p = path_locked();
        if (p.empty()) return;
        const std::string text = read_file(p);
        size_t pos = 0;
        while (pos < text.size()) {
            size_t nl = text.find('\n', pos);
            if (nl == std::string::npos) nl = text.size();
            std::string k;
            int one = -1;
            if (parse_step_line(text.substr(pos, nl - pos), k, one) && !steps_.count(k)) steps_[k] = one;
            pos = nl + 1;
        }
    }
    // Under mu_: queue one new kernel-form decision for the file.
    void queue_locked(const Entry& e) {
        const std::string p = path_locked();
        const std::string id = ident_of(std::get<0>(e.key));
        if (p.empty() || id.empty() || e.chosen < 0) return;
        queue_.push_back(line_of(id, e.key, e.chosen));
        queued_.store(true);
    }
    // The key a cache line replaces: kernel lines by DiskKey, step lines by
    // their step key; "" for a line that does not parse (dropped on rewrite).
    std::string line_key(const std::string& ln) const {
        DiskKey dk;
        int form = -1;
        std::string sk;
        int one = -1;
        if (parse_step_line(ln, sk, one)) return "S " + sk;
        if (!parse_line(ln, dk, form)) return std::string();
        char buf[512];
        snprintf(buf, sizeof(buf), "K %s %d %lld %s %lld %lld %d", std::get<0>(dk).c_str(), std::get<1>(dk),
                 (long long)std::get<2>(dk), std::get<3>(dk).c_str(), (long long)std::get<4>(dk),
                 (long long)std::get<5>(dk), std::get<6>(dk));
        return buf;
    }
    // Merge the queued lines into the file, outside mu_ (never fails the
    // caller, never blocks on the file lock for long): one thread of the
    // process at a time; flock(LOCK_NB) retried for at most ~50 ms, after
    // which the lines go back to the queue for a later call.
    void flush_persist() {
        if (!queued_.load()) return;
        std::unique_lock<std::mutex> io(io_mu_, std::try_to_lock);
        if (!io.owns_lock()) return;  // another thread is writing; it or a later call takes the queue
        std::vector<std::string> lines;
        std::string p;
        {
            std::lock_guard<std::mutex> lk(mu_);
            lines.swap(queue_);
            queued_.store(false);
            p = path_locked();
        }
        if (lines.empty() || p.empty()) return;
        bool written = false;
        make_dirs(p);
        const int lk = open((p + ".lock").c_str(), O_RDWR | O_CREAT | O_CLOEXEC, 0644);
        if (lk >= 0) {
            bool locked = false;
            for (int attempt = 0; attempt < 25 && !(locked = flock(lk, LOCK_EX | LOCK_NB) == 0); ++attempt)
                usleep(2000);
            if (locked) {
                // the new lines replace any line of the same key; every other line
                // that parses stays (other shapes, devices, processes); lines of
                // another ABI or format and corrupt lines go
                std::map<std::string, size_t> mine;
                for (size_t i = 0; i < lines.size(); ++i) {
                    std::string ln = lines[i];
                    if (!ln.empty() && ln.back() == '\n') ln.pop_back();
                    const std::string k = line_key(ln);
                    if (!k.empty()) mine[k] = i;  // the last decision of a key wins
                }
                std::string out;
                size_t kept = 0;
                const std::string text = read_file(p);
                size_t pos = 0;
                while (pos < text.size()) {
                    size_t nl = text.find('\n', pos);
                    if (nl == std::string::npos) nl = text.size();
                    const std::string ln = text.substr(pos, nl - pos);
                    const std::string k = line_key(ln);
                    if (!k.empty() && !mine.count(k) && kept + mine.size() < kCacheMaxLines) {
                        out += ln + "\n";
                        ++kept;
                    }
                    pos = nl + 1;
                }
                for (auto& kv : mine) out += lines[kv.second];
                char tmp_suffix[64];
                snprintf(tmp_suffix, sizeof(tmp_suffix), ".tmp.%ld", (long)getpid());
                const std::string tmp = p + tmp_suffix;
                FILE* f = fopen(tmp.c_str(), "wb");
                bool ok = f && fwrite(out.data(), 1, out.size(), f) == out.size();
                if (f) ok = (fclose(f) == 0) && ok;
                if (ok) ok = rename(tmp.c_str(), p.c_str()) == 0;
                if (!ok) (void)unlink(tmp.c_str());
                (void)flock(lk, LOCK_UN);
                written = true;  // a failed write is not retried (a read-only cache directory)
            }
            close(lk);
        } else {
            written = true;  // no lock file possible: the cache is unusable, drop the lines
        }
        if (!written) {
            std::lock_guard<std::mutex> g(mu_);
            queue_.insert(queue_.begin(), lines.begin(), lines.end());
            queued_.store(true);
        }
    }
    // Decide once the last candidate's end event has completed (the events
    // complete in stream order).  Under mu_.
    void harvest(Entry& e) {
        if (e.chosen >= 0 || !e.armed) return;
        const int n = (int)e.cand.size();
        // the second pass runs backwards: candidate 0's end event is the last one recorded
        const hipError_t q = hipEventQuery(e.events[2 * (size_t)n + 1]);
        if (q == hipErrorNotReady) return;
        std::vector<float> ms(n, 3.4e38f);  // per launch, the faster of the two passes
        bool ok = q == hipSuccess;
        for (int pass = 0; ok && pass < 2; ++pass)
            for (int c = 0; ok && c < n; ++c) {
                const size_t i = 2 * ((size_t)pass * n + c);
                float t = 0.f;
                if (hipEventElapsedTime(&t, e.events[i], e.events[i + 1]) != hipSuccess || !(t > 0.f)) ok = false;
                else if (t / (float)e.batch < ms[c]) ms[c] = t / (float)e.batch;
            }
        if (!ok) {
            (void)hipGetLastError();
            e.chosen = e.cand[0];
            release(e);
            return;
        }
        int b = 0;
        for (int c = 1; c < n; ++c)
            if (ms[c] < ms[b]) b = c;
        e.chosen = (ms[b] < kTuneMargin * ms[0]) ? e.cand[b] : e.cand[0];
        if (log_) {
            const int kind = std::get<1>(e.key);
            char line[1024];
            int k = snprintf(line, sizeof(line), "fedavg tuner: %s N=%lld P=%lld ldx=%lld%s batch=%d -> %s |",
                             kind == 1 ? "f32" : kind == 2 ? "bf16" : kind == 4 ? "f16" : "f32 rows", (long long)e.N,
                             (long long)std::get<4>(e.key), (long long)std::get<5>(e.key),
                             std::get<6>(e.key) ? " scored" : "", e.batch, form_name(kind, e.chosen));
            for (int c = 0; c < n && k > 0 && k < (int)sizeof(line); ++c)
                k += snprintf(line + k, sizeof(line) - k, " %s %.4f", form_name(kind, e.cand[c]), ms[c]);
            fprintf(stderr, "%s ms\n", line);
        }
        release(e);
        queue_locked(e);
    }
    const char* form_name(int kind, int form) const { return name_ ? name_(kind, form) : "?"; }
    FormName name_;
    FormFromName from_name_;
    DeviceIdent ident_;
    const int abi_;
    std::mutex mu_;
    std::map<Key, Entry> map_;
    std::map<DiskKey, int> preset_;         // decisions from the file / other processes
    std::map<std::string, bool> loaded_;    // device identities whose file lines are in preset_
    std::map<int, std::string> ident_cache_;
    std::map<std::string, int> steps_;      // step-form decisions: canonical key -> 1 one launch / 0 per round
    bool steps_loaded_ = false;
    std::vector<std::string> queue_;        // cache lines waiting for flush_persist
    std::atomic<bool> queued_{false};
    std::mutex io_mu_;                      // one file merge at a time in this process
    std::string path_;
    bool path_set_ = false;
    std::atomic<int> mode_{env_mode()};
    const bool log_ = getenv("FEDAVG_AUTOTUNE_LOG") && getenv("FEDAVG_AUTOTUNE_LOG")[0] == '1';
};

}  // namespace fa_tune
}  // namespace
