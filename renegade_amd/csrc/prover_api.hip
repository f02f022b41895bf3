// PRODUCT PATH — C-ABI implementation (include/rng_prover.h).
//
// Host orchestration for the MI355X prover backend: SRS load (ptau
// semantics of crates/circuits/circuit-types/src/primitives/srs.rs:63-214),
// NTT plans, MSM pipeline.  Single translation unit: includes the kernel
// files directly.
//
// The two prove functions here are the device choreography of their path
// only.  The round logic they share with each other and with rng_verify
// (per-proof state, blinder order, R4 + R5, linearization scalars,
// serialization, affine records) lives in plonk_rounds.hpp; the
// circuit-construction ABI lives in circuit_abi.hpp.
#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <functional>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <thread>
#include <vector>

#include "../../include/rng_prover.h"
#include "ntt_kernels.hip"
#include "msm_kernels.hip"
#include "lagrange_kernels.hip"
#include "plonk_kernels.hip"
#include "perm_kernels.hip"
#include "open_kernels.hip"
#include "plonk_circuit.hpp"
#include "plonk_host.hpp"
#include "plonk_rounds.hpp"
#include "test_circuits.hpp"
#include "circuits_core.hpp"
#include "pairing_impl.hpp"

namespace rng {

#define HIP_CHECK(x)                                                   \
    do {                                                               \
        hipError_t err__ = (x);                                        \
        if (err__ != hipSuccess) {                                     \
            fprintf(stderr, "rng_prover: HIP error %s at %s:%d\n",     \
                    hipGetErrorString(err__), __FILE__, __LINE__);     \
            return RNG_ERR_HIP;                                        \
        }                                                              \
    } while (0)

// every prover-path op runs on the calling thread's implicit stream so
// concurrent rng_prove calls from a thread pool overlap on the GPU
#define RNG_STREAM hipStreamPerThread

// Teardown guard: main-thread TLS / static / Python-GC destructors can run
// AFTER the HIP runtime's own atexit teardown, and a hipFree then faults
// inside the dead runtime (r01 bench exited rc=139 this way).  We register
// our atexit handler AFTER the first successful HIP call, so (LIFO order) it
// runs BEFORE the runtime's teardown and flips this flag; every destructor
// hipFree is gated on it.  Device memory skipped this way is reclaimed by
// process exit anyway.
static std::atomic<bool> g_hip_alive{true};
static bool hip_alive() { return g_hip_alive.load(std::memory_order_relaxed); }
static void hip_free_guarded(void* p) {
    if (p && hip_alive()) hipFree(p);
}

static bool gpu_ok() {
    static int cached = -1;
    if (cached < 0) {
        int n = 0;
        cached = (hipGetDeviceCount(&n) == hipSuccess && n > 0) ? 1 : 0;
        if (cached == 1)
            std::atexit([] { g_hip_alive.store(false, std::memory_order_relaxed); });
    }
    return cached == 1;
}

static thread_local double tls_msm_times[5] = {0, 0, 0, 0, 0};
static thread_local double tls_ntt_times[2] = {0, 0};

// Persistent host worker pool: parallelizes the per-proof host phases of
// cohort proving (grand product, evaluations, linearization) and the
// per-poly window folds of large fused MSM batches.  One job at a time;
// concurrent callers queue.  Never destroyed (leaked) so there is no
// thread-join ordering problem at process exit.
class HostPool {
    // Each job is a heap object shared by every thread that touches it: a
    // straggler from job A holds A's shared_ptr, sees A's exhausted `next`
    // counter and exits — it can never execute job B's indices with A's
    // (destroyed) callable.
    struct Job {
        std::function<void(uint32_t)> fn;
        uint32_t count;
        std::atomic<uint32_t> next{0}, done{0};
    };

  public:
    static HostPool& inst() {
        static HostPool* p = new HostPool();  // leaked: no join-at-exit problem
        return *p;
    }

    void parallel_for(uint32_t count, const std::function<void(uint32_t)>& fn) {
        if (count == 0) return;
        if (count == 1 || workers_.empty()) {
            for (uint32_t i = 0; i < count; ++i) fn(i);
            return;
        }
        std::unique_lock<std::mutex> job_lk(job_mu_);  // one job at a time
        auto job = std::make_shared<Job>();
        job->fn = fn;
        job->count = count;
        {
            std::lock_guard<std::mutex> lk(mu_);
            job_ = job;
            ++generation_;
        }
        cv_.notify_all();
        run_job(*job);  // caller participates
        {
            std::unique_lock<std::mutex> lk(mu_);
            done_cv_.wait(lk, [&] {
                return job->done.load(std::memory_order_acquire) >= count;
            });
            job_.reset();
        }
    }

  private:
    HostPool() {
        unsigned n = std::thread::hardware_concurrency();
        if (n == 0) n = 4;
        if (n > 32) n = 32;
        for (unsigned t = 0; t + 1 < n; ++t)
            workers_.emplace_back([this] { worker_loop(); });
    }
    void run_job(Job& job) {
        for (;;) {
            uint32_t i = job.next.fetch_add(1, std::memory_order_relaxed);
            if (i >= job.count) break;
            job.fn(i);
            if (job.done.fetch_add(1, std::memory_order_acq_rel) + 1 >= job.count) {
                std::lock_guard<std::mutex> lk(mu_);
                done_cv_.notify_all();
            }
        }
    }
    void worker_loop() {
        uint64_t seen = 0;
        for (;;) {
            std::shared_ptr<Job> job;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return generation_ != seen || stopping_; });
                if (stopping_) return;
                seen = generation_;
                job = job_;
            }
            if (job) run_job(*job);
        }
    }
    std::mutex job_mu_;
    std::mutex mu_;
    std::condition_variable cv_, done_cv_;
    std::vector<std::thread> workers_;
    std::shared_ptr<Job> job_;
    uint64_t generation_ = 0;
    bool stopping_ = false;

  public:
    // Join every worker (profilers' finalizers can stall on foreign live
    // threads at process exit; bench/debug scripts call rng_shutdown_pool
    // before exiting under rocprof).  parallel_for falls back to serial
    // execution afterwards.
    void stop() {
        std::unique_lock<std::mutex> job_lk(job_mu_);
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (stopping_) return;
            stopping_ = true;
        }
        cv_.notify_all();
        for (auto& t : workers_) t.join();
        workers_.clear();
    }
};

struct EvtTimer {
    hipEvent_t ev[8];
    int used = 0;
    EvtTimer() {
        for (auto& e : ev) hipEventCreate(&e);
    }
    ~EvtTimer() {
        for (auto& e : ev) hipEventDestroy(e);
    }
    void mark(hipStream_t s) {
        if (used < 8) hipEventRecord(ev[used++], s);
    }
    void collect(double* out, int n) {
        hipEventSynchronize(ev[used - 1]);
        for (int i = 0; i < n && i + 1 < used; ++i) {
            float ms = 0;
            hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
            out[i] = ms;
        }
    }
};

// ---------------- NTT plans ----------------

struct NttPlan {
    uint32_t n, logn, N1, N2, logN1, logN2, split_log;
    // device tables (fwd, inv): stage tables for len N1 and N2, outer TA/TB
    Fr *wst1_f = nullptr, *wst2_f = nullptr, *ta_f = nullptr, *tb_f = nullptr;
    Fr *wst1_i = nullptr, *wst2_i = nullptr, *ta_i = nullptr, *tb_i = nullptr;
    Fr ninv;  // Montgomery form
    Fr* scratch = nullptr;  // n elements, for the pass-2 ping-pong (resized w/ batch)
    uint64_t scratch_elems = 0;
    // coset tables (built on demand): gpow g^j, gpow_inv g^-j, xpow g*w^j
    Fr *gpow = nullptr, *gpow_inv = nullptr, *xpow = nullptr;
};

// host-side helpers over the shared field type (host-compiled path of Fp4)
static Fr h_fr_root_of_unity(uint32_t n) {
    static const u64 root_c[4] = FR_TWO_ADIC_ROOT;
    Fr root = Fr::from_canonical(root_c);
    uint32_t logn = 0;
    while ((1u << logn) < n) logn++;
    for (uint32_t i = logn; i < FR_TWO_ADICITY; ++i) root = root.sqr();
    return root;
}

struct RngCtxImpl {
    // SRS
    std::vector<uint64_t> srs_g1_host;  // (max_degree+1) * 8 u64 packed affine
    uint64_t srs_count = 0;
    void* srs_dev = nullptr;
    // fixed-base window tables T[j*srs_count + i] = 2^(c*j) * P_i, built
    // lazily per window size c (msm_fixed_c returns at most three values)
    struct FixedTable {
        uint32_t c = 0;
        void* dev = nullptr;
    };
    FixedTable fixed_tables[3];
    // direct-lookup tables L[((w*N + i) << (c-1)) + d-1] = d * 2^(c*w) * P_i
    // for c = 8, 9, 10 (slot c - 8), built lazily under mu from the window
    // table of the same c.  `tried` keeps a table that did not fit the budget
    // or the free memory, or whose build failed, from being tried again.
    struct LookupTable {
        void* dev = nullptr;
        bool tried = false;
    };
    LookupTable lookup_tables[3];
    // Lagrange bases per domain size n: n + 2 affine points
    // [L_0(tau)] .. [L_{n-1}(tau)], [tau^n] - [tau^0], [tau^(n+1)] - [tau^1],
    // and their window tables for at most two window sizes.  Built lazily
    // under mu; an unusable domain (a base at infinity, n + 2 > srs_count,
    // a failed build) keeps its entry so it is not tried again.
    // lookup[c - 8]: the direct-lookup table over the domain's bases, rows
    // (w, i) of the window table of the same c, for the sum over compacted
    // entries; budget and `tried` as for lookup_tables.
    struct LagrangeDomain {
        bool usable = false;
        void* bases = nullptr;
        FixedTable tables[2];
        LookupTable lookup[3];
    };
    std::map<uint64_t, LagrangeDomain> lagrange;
    uint64_t h_g2[16];       // h: x.c0,x.c1,y.c0,y.c1 Montgomery
    uint64_t beta_h_g2[16];
    std::map<uint32_t, std::unique_ptr<NttPlan>> plans;
    std::mutex mu;

    ~RngCtxImpl() {
        for (auto& kv : plans) {
            NttPlan* p = kv.second.get();
            for (Fr* b : {p->wst1_f, p->wst2_f, p->ta_f, p->tb_f, p->wst1_i,
                          p->wst2_i, p->ta_i, p->tb_i, p->scratch, p->gpow,
                          p->gpow_inv, p->xpow})
                hip_free_guarded(b);
        }
        hip_free_guarded(srs_dev);
        for (auto& t : fixed_tables) hip_free_guarded(t.dev);
        for (auto& t : lookup_tables) hip_free_guarded(t.dev);
        for (auto& kv : lagrange) {
            hip_free_guarded(kv.second.bases);
            for (auto& t : kv.second.tables) hip_free_guarded(t.dev);
            for (auto& t : kv.second.lookup) hip_free_guarded(t.dev);
        }
    }
};

static int build_pow_table(Fr** out, const Fr& base, uint64_t step, uint64_t count) {
    HIP_CHECK(hipMalloc(out, count * sizeof(Fr)));
    uint32_t blocks = (uint32_t)((count + 255) / 256);
    hipLaunchKernelGGL(k_pow_table, dim3(blocks), dim3(256), 0, 0, *out, base, step, count);
    HIP_CHECK(hipGetLastError());
    return RNG_OK;
}

// single-workgroup NTT threshold: one WG per column is latency-bound (12
// serial stages), so route n >= 2048 through the two-pass col/row path
// (64-wide grids) — measured 3x faster at n=4096 (the proof domain).
static constexpr uint32_t NTT_SMALL_MAX = 1024;
// largest transform: the row pass stages N1 = 2^ceil(logn/2) elements in one
// workgroup's LDS, and 2^24 (N1 = 4096, 128 KiB) is the last size whose row
// fits the 160 KiB a workgroup has; 2^25 would ask for 256 KiB.  The
// 128 KiB dynamic request is granted by the plain launch below
// (tests/test_ntt_tiers.py compares 2^23 and 2^24 in full).
static constexpr uint64_t NTT_MAX_N = 1ull << 24;
// filled 256-thread blocks for passes with N <= 256 (log2 n 11..17), decided
// by the headline A/B of profiles/ntt_filled_blocks_ab.json
static constexpr bool NTT_FILL_DEFAULT = true;

// public-API argument contract (include/rng_prover.h), checked before any
// allocation, copy or plan construction
static bool ntt_args_ok(uint64_t n, uint64_t batch) {
    return n >= 2 && !(n & (n - 1)) && n <= NTT_MAX_N && batch >= 1;
}

static NttPlan* get_plan(RngCtxImpl* ctx, uint32_t n, uint64_t batch) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto it = ctx->plans.find(n);
    NttPlan* p;
    if (it != ctx->plans.end()) {
        p = it->second.get();
    } else {
        auto np = std::make_unique<NttPlan>();
        p = np.get();
        p->n = n;
        p->logn = 0;
        while ((1u << p->logn) < n) p->logn++;
        p->logN2 = p->logn / 2;
        p->logN1 = p->logn - p->logN2;
        p->N1 = 1u << p->logN1;
        p->N2 = 1u << p->logN2;
        p->split_log = p->logN2 < 6 ? p->logN2 : 6;
        Fr w = h_fr_root_of_unity(n);
        Fr wi = w.inverse();
        Fr wN1_f = w.pow_u64(p->N2), wN2_f = w.pow_u64(p->N1);
        Fr wN1_i = wi.pow_u64(p->N2), wN2_i = wi.pow_u64(p->N1);
        uint64_t split = 1ull << p->split_log;
        if (n <= NTT_SMALL_MAX) {
            // single-WG path needs only the full-length stage table (in wst1)
            if (build_pow_table(&p->wst1_f, w, 1, n / 2) != RNG_OK) return nullptr;
            if (build_pow_table(&p->wst1_i, wi, 1, n / 2) != RNG_OK) return nullptr;
        } else {
            if (build_pow_table(&p->wst1_f, wN1_f, 1, p->N1 / 2) != RNG_OK) return nullptr;
            if (build_pow_table(&p->wst2_f, wN2_f, 1, p->N2 / 2) != RNG_OK) return nullptr;
            if (build_pow_table(&p->ta_f, w, split, (uint64_t)p->N1 * (p->N2 >> p->split_log)) != RNG_OK) return nullptr;
            if (build_pow_table(&p->tb_f, w, 1, (uint64_t)p->N1 * split) != RNG_OK) return nullptr;
            if (build_pow_table(&p->wst1_i, wN1_i, 1, p->N1 / 2) != RNG_OK) return nullptr;
            if (build_pow_table(&p->wst2_i, wN2_i, 1, p->N2 / 2) != RNG_OK) return nullptr;
            if (build_pow_table(&p->ta_i, wi, split, (uint64_t)p->N1 * (p->N2 >> p->split_log)) != RNG_OK) return nullptr;
            if (build_pow_table(&p->tb_i, wi, 1, (uint64_t)p->N1 * split) != RNG_OK) return nullptr;
        }
        u64 nc[4] = {n, 0, 0, 0};
        p->ninv = Fr::from_canonical(nc).inverse();
        if (hipDeviceSynchronize() != hipSuccess) return nullptr;
        ctx->plans.emplace(n, std::move(np));
    }
    if (n > NTT_SMALL_MAX && p->scratch_elems < (uint64_t)n * batch) {
        if (p->scratch) hipFree(p->scratch);
        if (hipMalloc(&p->scratch, (uint64_t)n * batch * sizeof(Fr)) != hipSuccess) {
            p->scratch = nullptr;
            p->scratch_elems = 0;
            return nullptr;
        }
        p->scratch_elems = (uint64_t)n * batch;
    }
    return p;
}

// out-of-place for n > NTT_SMALL_MAX (result in out); in-place for small n.
static int ntt_dev_run(RngCtxImpl* ctx, Fr* data, Fr* out, uint32_t n, uint64_t batch,
                       bool inverse, hipStream_t stream = 0) {
    // batch=0 to get_plan: tables only — ntt_dev_run never touches the
    // plan's public-API scratch (rng_ntt_fr_dev sizes it itself)
    NttPlan* p = get_plan(ctx, n, 0);
    if (!p) return RNG_ERR_HIP;
    if (n <= NTT_SMALL_MAX) {
        Fr* wst = inverse ? p->wst1_i : p->wst1_f;
        hipLaunchKernelGGL(k_ntt_small, dim3((uint32_t)batch), dim3(512), n * sizeof(Fr),
                           stream, data, wst, n, p->logn, p->ninv, inverse ? 1 : 0);
        HIP_CHECK(hipGetLastError());
        if (out != data)
            HIP_CHECK(hipMemcpyAsync(out, data, (uint64_t)n * batch * sizeof(Fr),
                                     hipMemcpyDeviceToDevice, stream));
        return RNG_OK;
    }
    Fr* wst1 = inverse ? p->wst1_i : p->wst1_f;
    Fr* wst2 = inverse ? p->wst2_i : p->wst2_f;
    Fr* ta = inverse ? p->ta_i : p->ta_f;
    Fr* tb = inverse ? p->tb_i : p->tb_f;
    // pair width per pass: 2 (64-byte-coalesced global access) while the
    // pair fits 64 KiB LDS (>=2 blocks/CU); above that, singles — at 2^22
    // the 128 KiB pair form pinned the DFT at 1 block/CU and the dependent
    // butterfly muls ran latency-exposed
    static uint32_t pw_lds_cap = [] {
        const char* e = getenv("RNG_NTT_PAIR_LDS");  // A/B knob, bytes
        return e ? (uint32_t)atoi(e) : 65536u;
    }();
    // filled blocks for passes with N <= 256 (ntt_kernels.hip): PW = 512 / N
    // columns (rows) per 256-thread block.  RNG_NTT_FILL=0 keeps the 512-thread
    // pair kernels at every size, for A/B runs
    static const bool fill = [] {
        const char* e = getenv("RNG_NTT_FILL");
        return e ? atoi(e) != 0 : NTT_FILL_DEFAULT;
    }();
    const uint32_t fpw1 = NTT_FILL_ELEMS / p->N2, fpw2 = NTT_FILL_ELEMS / p->N1;
    const bool fill1 = fill && fpw1 >= 2 && fpw1 <= p->N1;
    const bool fill2 = fill && fpw2 >= 2 && fpw2 <= p->N2;
    const uint32_t pw1 = (2u * p->N2 * sizeof(Fr) <= pw_lds_cap) ? 2 : 1;
    const uint32_t pw2 = (2u * p->N1 * sizeof(Fr) <= pw_lds_cap) ? 2 : 1;
    uint32_t lds1 = pw1 * p->N2 * sizeof(Fr);
    uint32_t lds2 = pw2 * p->N1 * sizeof(Fr);
    EvtTimer et;
    et.mark(stream);
    if (fill1)
        hipLaunchKernelGGL(k_ntt_col_fill, dim3((uint32_t)(p->N1 / fpw1 * batch)),
                           dim3(NTT_FILL_THREADS), NTT_FILL_ELEMS * sizeof(Fr), stream, data,
                           wst2, ta, tb, p->N1, p->N2, p->logN2, p->split_log,
                           (uint32_t)__builtin_ctz(fpw1));
    else if (pw1 == 2)
        hipLaunchKernelGGL(k_ntt_col<2>, dim3((uint32_t)(p->N1 / 2 * batch)), dim3(512),
                           lds1, stream, data, wst2, ta, tb, p->N1, p->N2, p->logN2,
                           p->split_log);
    else
        hipLaunchKernelGGL(k_ntt_col<1>, dim3((uint32_t)(p->N1 * batch)), dim3(512),
                           lds1, stream, data, wst2, ta, tb, p->N1, p->N2, p->logN2,
                           p->split_log);
    HIP_CHECK(hipGetLastError());
    et.mark(stream);
    if (fill2)
        hipLaunchKernelGGL(k_ntt_row_fill, dim3((uint32_t)(p->N2 / fpw2 * batch)),
                           dim3(NTT_FILL_THREADS), NTT_FILL_ELEMS * sizeof(Fr), stream, data,
                           out, wst1, p->N1, p->N2, p->logN1, (uint32_t)__builtin_ctz(fpw2),
                           p->ninv, inverse ? 1 : 0);
    else if (pw2 == 2)
        hipLaunchKernelGGL(k_ntt_row<2>, dim3((uint32_t)(p->N2 / 2 * batch)), dim3(512),
                           lds2, stream, data, out, wst1, p->N1, p->N2, p->logN1,
                           p->ninv, inverse ? 1 : 0);
    else
        hipLaunchKernelGGL(k_ntt_row<1>, dim3((uint32_t)(p->N2 * batch)), dim3(512),
                           lds2, stream, data, out, wst1, p->N1, p->N2, p->logN1,
                           p->ninv, inverse ? 1 : 0);
    HIP_CHECK(hipGetLastError());
    et.mark(stream);
    et.collect(tls_ntt_times, 2);
    return RNG_OK;
}

// ---------------- MSM ----------------

// The RNG_MSM_* variables, read once per process.  RNG_MSM_FIXED=0 sends
// SRS commitments down the windowed path for A/B runs; the others are
// tuning overrides that apply only inside the range given (0 = unset).
struct MsmEnv {
    int fixed;    // RNG_MSM_FIXED, default 1
    int c;        // RNG_MSM_C 8..16: window size, only where window_c == 0
    int chunk;    // RNG_MSM_CHUNK 2..16: buckets per window-sum lane
    int subb;     // RNG_MSM_SUBB 1..256: combine sub-blocks per key group
    int seg_cap;  // RNG_MSM_SEGCAP 8..MSM_MAX_SEG: fixed-base sub-segment cap
    int debug;    // RNG_MSM_DEBUG: one stderr line per MSM
    // direct-lookup path
    int lookup;         // RNG_MSM_LOOKUP: 0 never, 1 wherever a table fits, -1 unset
    int lookup_max_mb;  // RNG_MSM_LOOKUP_MAX_MB: table byte budget, default 10 GiB
    int lookup_c;       // RNG_MSM_LOOKUP_C 8..10: the selector's window size
    int lookup_l;       // RNG_MSM_LOOKUP_L 1..8: scalars per lane
    // lookup sum over compacted entries, round 1
    int r1_lookup;    // RNG_R1_LOOKUP: 0 off, 1 on, -1 unset (R1_LOOKUP_DEFAULT)
    int r1_lookup_s;  // RNG_R1_LOOKUP_S 1..64: blocks per poly
};

static const MsmEnv& msm_env() {
    static const MsmEnv env = [] {
        auto get = [](const char* name, int unset) {
            const char* e = getenv(name);
            return e ? atoi(e) : unset;
        };
        return MsmEnv{get("RNG_MSM_FIXED", 1),  get("RNG_MSM_C", 0),
                      get("RNG_MSM_CHUNK", 0),  get("RNG_MSM_SUBB", 0),
                      get("RNG_MSM_SEGCAP", 0), get("RNG_MSM_DEBUG", 0),
                      get("RNG_MSM_LOOKUP", -1), get("RNG_MSM_LOOKUP_MAX_MB", 10240),
                      get("RNG_MSM_LOOKUP_C", 0), get("RNG_MSM_LOOKUP_L", 0),
                      get("RNG_R1_LOOKUP", -1), get("RNG_R1_LOOKUP_S", 0)};
    }();
    return env;
}

// The prover's own switches, read once per process.  z_device, r1_lagrange
// and open_device: -1 = unset (Z_DEVICE_DEFAULT, R1_LAGRANGE_MIN_K and
// OPEN_DEVICE_DEFAULT decide), 0 = off, 1 = on, for every k.
struct ProverEnv {
    int z_device;      // RNG_Z_DEVICE: R2 grand product on the device
    int r1_lagrange;   // RNG_R1_LAGRANGE: R1 commits in the Lagrange basis
    int open_device;   // RNG_OPEN_DEVICE: R4 + R5 on the device
    int cohort_trace;  // RNG_COHORT_TRACE: stderr timeline of a cohort
    static bool on(int v, bool path_default) { return v < 0 ? path_default : v == 1; }
};

static const ProverEnv& prover_env() {
    static const ProverEnv env = [] {
        auto tri = [](const char* name) {
            const char* e = getenv(name);
            return e ? (atoi(e) != 0 ? 1 : 0) : -1;
        };
        const char* t = getenv("RNG_COHORT_TRACE");
        return ProverEnv{tri("RNG_Z_DEVICE"), tri("RNG_R1_LAGRANGE"), tri("RNG_OPEN_DEVICE"),
                         t ? atoi(t) : 0};
    }();
    return env;
}

// What an MSM gathers its points from: a plain base array (windowed
// Pippenger, one bucket set per (poly, window)), or the fixed-base window
// table T[j*stride + i] = 2^(c*j) * P_i built for this c (every digit
// gathers its own pre-weighted point, so a poly's W digit positions share
// ONE bucket set and the fold sees a single "window").
struct MsmBases {
    const G1Aff* points;    // base array, or the window table
    uint64_t table_stride;  // 0 = plain base array; else the table's row length N
    static MsmBases plain(const G1Aff* bases) { return {bases, 0}; }
    static MsmBases table(const G1Aff* t, uint64_t stride) { return {t, stride}; }
    bool fixed() const { return table_stride != 0; }
};

// Every size of one MSM call: B polys of n scalars at window size c.
struct MsmShape {
    uint64_t n;
    uint32_t B, c;
    bool fixed;
    bool compact;        // write and sort only the non-zero digits (Lagrange path)
    uint32_t Wd;         // digit positions per scalar
    uint32_t W;          // windows per poly as seen by buckets/aggregation/fold
    uint32_t G;          // key groups
    uint32_t key_shift;  // keys pack group << key_shift | magnitude
    uint64_t total;      // digit entries
    uint64_t nb;         // buckets
    uint32_t chunk_sz;   // buckets per window-sum lane
    uint64_t nchunks;
    uint32_t cw;         // chunks per key group
    uint32_t subb;       // combine sub-blocks per key group
    uint32_t seg_cap;    // longest sub-segment one reduce lane walks
    uint32_t sentinel;   // key of a zero digit
    uint32_t sort_bits;  // live key bits
};

static MsmShape msm_shape(uint64_t n, uint32_t B, uint32_t c, bool fixed,
                          bool compact = false) {
    const MsmEnv& env = msm_env();
    MsmShape sh;
    sh.n = n;
    sh.B = B;
    sh.c = c;
    sh.fixed = fixed;
    sh.compact = compact;
    sh.Wd = (256 + c - 1) / c;
    sh.W = fixed ? 1 : sh.Wd;
    sh.G = B * sh.W;
    // the fixed mode packs tightly (magnitude <= 2^(c-1) needs c bits) so the
    // sort touches c + gb bits
    sh.key_shift = fixed ? c : 16;
    sh.total = n * B * sh.Wd;
    sh.nb = (1ull << (c - 1)) * sh.G;
    // chunk size adapts to keep the window-sum stages wide: small MSMs (few
    // windows x small bucket counts) get chunk=2 (4x the lanes, 4x shorter
    // latency chains), the 2^20 leg keeps chunk=16.
    // target >=128k lanes: the per-chunk suffix walk is a serial EC chain, so
    // the chunk kernel is latency-bound until the chip is several waves deep
    // per SIMD (r02: chunk 16 -> 4 at 2^20 cut window_chunks ~3x)
    sh.chunk_sz = MSM_CHUNK;
    while (sh.chunk_sz > 2 && sh.nb / sh.chunk_sz < 131072) sh.chunk_sz >>= 1;
    if (env.chunk >= 2 && env.chunk <= 16) sh.chunk_sz = (uint32_t)env.chunk;
    if ((1u << (c - 1)) < sh.chunk_sz) sh.chunk_sz = 1u << (c - 1);
    sh.nchunks = ((1ull << (c - 1)) / sh.chunk_sz) * sh.G;
    sh.cw = (1u << (c - 1)) / sh.chunk_sz;
    // sub-blocks per window: enough blocks to spread chunks, but never more
    // than chunks (idle blocks)
    sh.subb = MSM_SUBB;
    while (sh.subb > 1 && sh.cw / sh.subb < 64) sh.subb >>= 1;
    // the combine blocks are serial EC chains: push toward >=2048 waves
    // (1 block = 1 wave of 64 lanes) while keeping >=64 chunks per block
    // so the scan-based combine2 applies
    while (sh.subb < 256 && sh.G * sh.subb < 4096 && sh.cw / (2 * sh.subb) >= 64 &&
           (uint64_t)sh.G * sh.subb * 2 <= 8192)
        sh.subb <<= 1;
    if (env.subb >= 1 && env.subb <= 256) sh.subb = (uint32_t)env.subb;
    // fixed-base mode: a bucket holds n*W/2^(c-1) entries (W times the
    // windowed path's), so the cap trades bucket-reduce lanes against
    // Jacobian adds in k_msm_seg_merge; only there does the override apply
    sh.seg_cap = msm_seg_cap(sh.total);
    if (fixed && env.seg_cap >= 8 && env.seg_cap <= (int)MSM_MAX_SEG)
        sh.seg_cap = (uint32_t)env.seg_cap;
    // sort only the live key bits: the magnitude bits (16, or c in fixed-base
    // mode) + enough for G groups + the sentinel (G << key_shift)
    uint32_t gb = 1;
    while ((1u << gb) <= sh.G) ++gb;
    sh.sentinel = sh.G << sh.key_shift;
    sh.sort_bits = sh.key_shift + gb;
    return sh;
}

struct MsmScratch {
    uint32_t *keys_in = nullptr, *keys_out = nullptr, *vals_in = nullptr, *vals_out = nullptr;
    void* sort_temp = nullptr;
    size_t sort_temp_bytes = 0;
    uint8_t* head_flags = nullptr;
    uint32_t* heads = nullptr;
    uint32_t* lens = nullptr;
    uint32_t* nsub = nullptr;
    uint32_t* sub_off = nullptr;
    uint32_t* sub_start = nullptr;
    uint32_t* sub_len = nullptr;
    uint32_t* sub_len_sorted = nullptr;
    uint32_t* sub_order = nullptr;
    uint32_t* nsub_sorted = nullptr;
    uint32_t* head_order = nullptr;
    G1Jac* partials2 = nullptr;
    uint32_t* head_count = nullptr;  // device u32
    void* select_temp = nullptr;
    size_t select_temp_bytes = 0;
    void* scan_temp = nullptr;
    size_t scan_temp_bytes = 0;
    G1Jac* buckets = nullptr;
    G1Jac* partials = nullptr;
    G1Jac* window_sums = nullptr;
    uint64_t window_sums_cap = 0;  // entries (G*subb grows with fused B)
    G1Jac* result = nullptr;
    uint64_t cap_entries = 0;
    uint64_t cap_nb = 0;
    uint64_t cap_nchunks = 0;
    uint64_t last_entries = 0;  // entries the last run sorted (RNG_MSM_DEBUG)

    ~MsmScratch() {
        for (void* b : {(void*)keys_in, (void*)keys_out, (void*)vals_in, (void*)vals_out,
                        sort_temp, (void*)head_flags, (void*)heads, (void*)lens,
                        (void*)nsub, (void*)sub_off, (void*)sub_start, (void*)sub_len,
                        (void*)sub_len_sorted, (void*)sub_order,
                        (void*)nsub_sorted, (void*)head_order,
                        (void*)partials2, (void*)head_count, select_temp, scan_temp,
                        (void*)buckets, (void*)partials, (void*)window_sums,
                        (void*)result})
            hip_free_guarded(b);
    }
};

static thread_local std::unique_ptr<MsmScratch> tls_msm_scratch;

// The calling thread's scratch, grown to hold `sh`.
static int msm_scratch_ensure(const MsmShape& sh, hipStream_t stream, MsmScratch** out) {
    if (!tls_msm_scratch) tls_msm_scratch = std::make_unique<MsmScratch>();
    MsmScratch* s = tls_msm_scratch.get();
    if (s->cap_entries < sh.total || s->cap_nb < sh.nb || s->cap_nchunks < sh.nchunks) {
        // size with 1.5x slack so nearby problem sizes (n, n+2, n+3 commits,
        // different auto window sizes) never thrash device allocations
        uint64_t cap_total = sh.total + sh.total / 2 + 64;
        uint64_t cap_nb2 = sh.nb + sh.nb / 2 + 64;
        uint64_t cap_nch = sh.nchunks + sh.nchunks / 2 + 64;
        // never shrink a dimension: shapes that alternate on one thread (the
        // Lagrange round at c=8: many entries, few buckets; the dense rounds
        // at c=13: the reverse) would otherwise reallocate on every call
        if (cap_total < s->cap_entries) cap_total = s->cap_entries;
        if (cap_nb2 < s->cap_nb) cap_nb2 = s->cap_nb;
        if (cap_nch < s->cap_nchunks) cap_nch = s->cap_nchunks;
        tls_msm_scratch = std::make_unique<MsmScratch>();
        s = tls_msm_scratch.get();
        HIP_CHECK(hipMalloc(&s->keys_in, cap_total * 4));
        HIP_CHECK(hipMalloc(&s->keys_out, cap_total * 4));
        HIP_CHECK(hipMalloc(&s->vals_in, cap_total * 4));
        HIP_CHECK(hipMalloc(&s->vals_out, cap_total * 4));
        rocprim::radix_sort_pairs(nullptr, s->sort_temp_bytes, s->keys_in, s->keys_out,
                                  s->vals_in, s->vals_out, cap_total, 0, 27, stream);
        HIP_CHECK(hipMalloc(&s->sort_temp, s->sort_temp_bytes));
        HIP_CHECK(hipMalloc(&s->head_flags, cap_total));
        uint64_t max_heads_cap = (cap_nb2 < cap_total ? cap_nb2 : cap_total) + 1;
        uint64_t max_subs_cap = max_heads_cap + cap_total / 8 + 1;
        HIP_CHECK(hipMalloc(&s->heads, max_heads_cap * 4));
        HIP_CHECK(hipMalloc(&s->lens, max_heads_cap * 4));
        HIP_CHECK(hipMalloc(&s->nsub, max_heads_cap * 4));
        HIP_CHECK(hipMalloc(&s->sub_off, max_heads_cap * 4));
        HIP_CHECK(hipMalloc(&s->sub_start, max_subs_cap * 4));
        HIP_CHECK(hipMalloc(&s->sub_len, max_subs_cap * 4));
        HIP_CHECK(hipMalloc(&s->sub_len_sorted, max_subs_cap * 4));
        HIP_CHECK(hipMalloc(&s->sub_order, max_subs_cap * 4));
        HIP_CHECK(hipMalloc(&s->nsub_sorted, max_heads_cap * 4));
        HIP_CHECK(hipMalloc(&s->head_order, max_heads_cap * 4));
        HIP_CHECK(hipMalloc(&s->partials2, max_subs_cap * sizeof(G1Jac)));
        HIP_CHECK(hipMalloc(&s->head_count, 4));
        {
            rocprim::counting_iterator<uint32_t> cit(0);
            uint64_t sel_cap = cap_total > cap_nb2 ? cap_total : cap_nb2;
            (void)rocprim::select(nullptr, s->select_temp_bytes, cit, s->head_flags,
                                  s->heads, s->head_count, sel_cap, stream);
            HIP_CHECK(hipMalloc(&s->select_temp, s->select_temp_bytes));
            // also covers the compacted path's scan over per-scalar counts
            uint64_t scan_cap = max_heads_cap > cap_nb2 ? max_heads_cap : cap_nb2;
            if (scan_cap < cap_total) scan_cap = cap_total;
            (void)rocprim::exclusive_scan(nullptr, s->scan_temp_bytes, s->nsub,
                                          s->sub_off, 0u, scan_cap,
                                          rocprim::plus<uint32_t>(), stream);
            HIP_CHECK(hipMalloc(&s->scan_temp, s->scan_temp_bytes));
        }
        HIP_CHECK(hipMalloc(&s->buckets, cap_nb2 * sizeof(G1Jac)));
        HIP_CHECK(hipMalloc(&s->partials, 2 * cap_nch * sizeof(G1Jac)));
        HIP_CHECK(hipMalloc(&s->window_sums, 512 * MSM_SUBB * sizeof(G1Jac)));
        s->window_sums_cap = 512 * MSM_SUBB;
        HIP_CHECK(hipMalloc(&s->result, sizeof(G1Jac)));
        s->cap_entries = cap_total;
        s->cap_nb = cap_nb2;
        s->cap_nchunks = cap_nch;
    }
    if ((uint64_t)sh.G * sh.subb > s->window_sums_cap) {
        // big fused batches (cohort k=64: G=10240 groups) outgrow the default
        // window_sums allocation.  null + zero first: a failed hipMalloc must
        // not leave a dangling pointer behind an inflated capacity
        hipFree(s->window_sums);
        s->window_sums = nullptr;
        s->window_sums_cap = 0;
        HIP_CHECK(hipMalloc(&s->window_sums, (uint64_t)sh.G * sh.subb * 2 * sizeof(G1Jac)));
        s->window_sums_cap = (uint64_t)sh.G * sh.subb * 2;
    }
    *out = s;
    return RNG_OK;
}

// Stage 1: digits -> radix sort -> segment heads -> capped sub-segments ->
// reduce -> merge.  Leaves one Jacobian per bucket in s->buckets.
static int msm_bucket_sums(MsmShape sh /* by value: the compacted path shrinks total */,
                           const MsmBases& bases, const uint64_t* d_scalars, MsmScratch* s,
                           EvtTimer& et, hipStream_t stream) {
    const uint32_t tb = 256;
    const uint32_t c = sh.c;
    const dim3 scalar_grid((uint32_t)((sh.n * sh.B + tb - 1) / tb));
    if (sh.compact) {
        // count -> exclusive scan -> scatter of the non-zero digits only.
        // counts and offsets borrow vals_out / keys_out, idle until the sort.
        const uint32_t ns = (uint32_t)(sh.n * sh.B);
        uint32_t *counts = s->vals_out, *offs = s->keys_out;
        hipLaunchKernelGGL(k_msm_digit_count, scalar_grid, dim3(tb), 0, stream, d_scalars,
                           ns, c, sh.Wd, counts);
        HIP_CHECK(hipGetLastError());
        (void)rocprim::exclusive_scan(s->scan_temp, s->scan_temp_bytes, counts, offs, 0u, ns,
                                      rocprim::plus<uint32_t>(), stream);
        hipLaunchKernelGGL(k_msm_digits_compact, scalar_grid, dim3(tb), 0, stream, d_scalars,
                           (uint32_t)sh.n, c, sh.Wd, sh.B, (uint32_t)bases.table_stride,
                           offs, s->keys_in, s->vals_in);
        HIP_CHECK(hipGetLastError());
        uint32_t last_off = 0, last_cnt = 0;
        HIP_CHECK(hipMemcpyAsync(&last_off, offs + ns - 1, 4, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipMemcpyAsync(&last_cnt, counts + ns - 1, 4, hipMemcpyDeviceToHost,
                                 stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        sh.total = (uint64_t)last_off + last_cnt;
        sh.seg_cap = msm_compact_seg_cap(sh.total);
        const int cap_env = msm_env().seg_cap;
        if (cap_env >= 8 && cap_env <= (int)MSM_MAX_SEG) sh.seg_cap = (uint32_t)cap_env;
        s->last_entries = sh.total;
        if (sh.total == 0) {  // every scalar zero: identity for every poly
            HIP_CHECK(hipMemsetAsync(s->buckets, 0, sh.nb * sizeof(G1Jac), stream));
            et.mark(stream);
            et.mark(stream);
            et.mark(stream);
            return RNG_OK;
        }
    } else if (sh.fixed)
        hipLaunchKernelGGL(k_msm_digits_fixed, scalar_grid, dim3(tb), 0, stream, d_scalars,
                           (uint32_t)sh.n, c, sh.Wd, sh.B, (uint32_t)bases.table_stride,
                           s->keys_in, s->vals_in);
    else
        hipLaunchKernelGGL(k_msm_digits, scalar_grid, dim3(tb), 0, stream, d_scalars,
                           (uint32_t)sh.n, c, sh.Wd, sh.B, s->keys_in, s->vals_in);
    HIP_CHECK(hipGetLastError());
    if (!sh.compact) s->last_entries = sh.total;
    const uint32_t total = (uint32_t)sh.total;
    et.mark(stream);
    rocprim::radix_sort_pairs(s->sort_temp, s->sort_temp_bytes, s->keys_in, s->keys_out,
                              s->vals_in, s->vals_out, sh.total, 0, sh.sort_bits, stream);
    HIP_CHECK(hipMemsetAsync(s->buckets, 0, sh.nb * sizeof(G1Jac), stream));
    hipLaunchKernelGGL(k_msm_head_flags, dim3((uint32_t)((sh.total + tb - 1) / tb)),
                       dim3(tb), 0, stream, s->keys_out, total, sh.sentinel, s->head_flags);
    HIP_CHECK(hipGetLastError());
    {
        rocprim::counting_iterator<uint32_t> cit(0);
        (void)rocprim::select(s->select_temp, s->select_temp_bytes, cit, s->head_flags,
                              s->heads, s->head_count, sh.total, stream);
    }
    uint64_t max_heads = sh.nb < sh.total ? sh.nb : sh.total;
    hipLaunchKernelGGL(k_msm_seg_lengths, dim3((uint32_t)((max_heads + tb - 1) / tb)),
                       dim3(tb), 0, stream, s->keys_out, s->heads, s->head_count, total,
                       s->lens, s->nsub, sh.seg_cap);
    HIP_CHECK(hipGetLastError());
    uint32_t hc = 0;
    HIP_CHECK(hipMemcpyAsync(&hc, s->head_count, 4, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    if (hc == 0) {  // every digit zero: the zeroed buckets are the answer
        et.mark(stream);
        et.mark(stream);
        return RNG_OK;
    }
    // sub-segment split (caps any lane's walk at seg_cap entries)
    (void)rocprim::exclusive_scan(s->scan_temp, s->scan_temp_bytes, s->nsub, s->sub_off, 0u,
                                  hc, rocprim::plus<uint32_t>(), stream);
    uint32_t last_off = 0, last_n = 0;
    HIP_CHECK(hipMemcpyAsync(&last_off, s->sub_off + hc - 1, 4, hipMemcpyDeviceToHost,
                             stream));
    HIP_CHECK(hipMemcpyAsync(&last_n, s->nsub + hc - 1, 4, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    uint32_t sub_total = last_off + last_n;
    hipLaunchKernelGGL(k_msm_make_subs, dim3((hc + tb - 1) / tb), dim3(tb), 0, stream,
                       s->heads, s->lens, s->sub_off, s->head_count, s->sub_start,
                       s->sub_len, sh.seg_cap);
    HIP_CHECK(hipGetLastError());
    {
        // order subs by length desc so each wave's lanes walk equal work
        rocprim::counting_iterator<uint32_t> cit(0);
        rocprim::radix_sort_pairs_desc(s->sort_temp, s->sort_temp_bytes, s->sub_len,
                                       s->sub_len_sorted, cit, s->sub_order, sub_total, 0,
                                       8, stream);
    }
    et.mark(stream);
    hipLaunchKernelGGL(k_msm_bucket_reduce, dim3((sub_total + tb - 1) / tb), dim3(tb), 0,
                       stream, s->vals_out, s->sub_start, s->sub_len, s->sub_order,
                       sub_total, bases.points, s->partials2);
    HIP_CHECK(hipGetLastError());
    {
        // order heads by sub count desc: the handful of long-merge heads
        // (top-window buckets) otherwise serialize whole waves
        rocprim::counting_iterator<uint32_t> cit(0);
        rocprim::radix_sort_pairs_desc(s->sort_temp, s->sort_temp_bytes, s->nsub,
                                       s->nsub_sorted, cit, s->head_order, hc, 0, 16,
                                       stream);
    }
    hipLaunchKernelGGL(k_msm_seg_merge, dim3((hc + tb - 1) / tb), dim3(tb), 0, stream,
                       s->keys_out, s->heads, s->sub_off, s->nsub, s->head_order, hc,
                       s->partials2, s->buckets, c, sh.key_shift);
    HIP_CHECK(hipGetLastError());
    et.mark(stream);
    return RNG_OK;
}

// Stage 2: per-chunk suffix sums of s->buckets, then the per-(group,
// sub-block) combine.  Leaves G*subb Jacobians in s->window_sums.
static int msm_window_sums(const MsmShape& sh, MsmScratch* s, EvtTimer& et,
                           hipStream_t stream) {
    const uint32_t tb = 256;
    hipLaunchKernelGGL(k_msm_window_chunks, dim3((uint32_t)((sh.nchunks + tb - 1) / tb)),
                       dim3(tb), 0, stream, s->buckets, sh.c, sh.G, sh.chunk_sz,
                       s->partials);
    HIP_CHECK(hipGetLastError());
    et.mark(stream);
    const bool scan2 = sh.cw % sh.subb == 0 && (sh.cw / sh.subb) % 64 == 0;
    if (msm_env().debug)
        fprintf(stderr,
                "[msm] n=%lu B=%u c=%u chunk=%u cw=%u subb=%u combine=%s entries=%lu%s\n",
                (unsigned long)sh.n, sh.B, sh.c, sh.chunk_sz, sh.cw, sh.subb,
                scan2 ? "scan2" : "v1", (unsigned long)s->last_entries,
                sh.compact ? " (compacted)" : "");
    if (scan2)  // scan-based combine: no per-chunk scalar weights
        hipLaunchKernelGGL(k_msm_window_combine2, dim3(sh.G * sh.subb), dim3(64), 0, stream,
                           s->partials, sh.c, sh.chunk_sz, sh.subb, s->window_sums);
    else
        hipLaunchKernelGGL(k_msm_window_combine, dim3(sh.G * sh.subb), dim3(64), 0, stream,
                           s->partials, sh.c, sh.chunk_sz, sh.subb, s->window_sums);
    HIP_CHECK(hipGetLastError());
    et.mark(stream);
    return RNG_OK;
}

// Stage 3, on the host (a single-lane dependent EC chain is far faster on a
// host core than on one GPU lane).  Two pooled steps: per-(poly, window)
// sub-block reduction, then the per-poly Horner across windows (the window
// count is small; a serial 1024-add fold on one core showed up at B=1 with
// wide subb).
static void msm_host_fold(const MsmShape& sh, const std::vector<G1Jac>& wsums,
                          G1Jac* h_result) {
    const uint32_t G = sh.G, W = sh.W, subb = sh.subb, c = sh.c;
    std::vector<G1Jac> wred((size_t)G);
    auto red_one = [&](uint32_t g) {
        G1Jac sum = wsums[(size_t)g * subb];
        for (uint32_t i = 1; i < subb; ++i) sum = sum.add(wsums[(size_t)g * subb + i]);
        wred[g] = sum;
    };
    auto fold_one = [&](uint32_t b) {
        G1Jac acc = wred[(size_t)b * W + W - 1];
        for (int w = (int)W - 2; w >= 0; --w) {
            for (uint32_t k = 0; k < c; ++k) acc = acc.dbl();
            acc = acc.add(wred[(size_t)b * W + w]);
        }
        h_result[b] = acc;
    };
    if ((uint64_t)G * subb >= 64)
        HostPool::inst().parallel_for(G, red_one);
    else
        for (uint32_t g = 0; g < G; ++g) red_one(g);
    if (sh.B >= 8)
        HostPool::inst().parallel_for(sh.B, fold_one);
    else
        for (uint32_t b = 0; b < sh.B; ++b) fold_one(b);
}

// B polynomials of n canonical scalars each (device) against one base
// description -> one fused pipeline; h_result[B].
static int msm_dev_run(const MsmBases& bases, const uint64_t* d_scalars, uint64_t n,
                       uint32_t c, G1Jac* h_result, uint32_t B = 1,
                       hipStream_t stream = RNG_STREAM, bool compact = false) {
    const MsmShape sh = msm_shape(n, B, c, bases.fixed(), compact && bases.fixed());
    MsmScratch* s = nullptr;
    int rc = msm_scratch_ensure(sh, stream, &s);
    if (rc != RNG_OK) return rc;
    // six marks -> tls_msm_times: digits, sort (to the reduce launch),
    // bucket_reduce (+ merge), window_chunks, final (combine)
    EvtTimer et;
    et.mark(stream);
    if ((rc = msm_bucket_sums(sh, bases, d_scalars, s, et, stream)) != RNG_OK) return rc;
    if ((rc = msm_window_sums(sh, s, et, stream)) != RNG_OK) return rc;
    std::vector<G1Jac> wsums((size_t)sh.G * sh.subb);
    HIP_CHECK(hipMemcpyAsync(wsums.data(), s->window_sums,
                             sh.G * sh.subb * sizeof(G1Jac), hipMemcpyDeviceToHost,
                             stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    et.collect(tls_msm_times, 5);
    msm_host_fold(sh, wsums, h_result);
    return RNG_OK;
}

// ---- fixed-base MSM over the SRS ----
// RNG_MSM_FIXED=0 restores the windowed (variable-base) path for A/B runs
static inline bool msm_fixed_enabled() { return msm_env().fixed != 0; }

// Window table for window size c, built on first use.  Returns nullptr when
// no table is allowed (over 1 GiB, index past 31 bits, all three slots taken
// by other window sizes) or the build failed; callers then fall back to the
// windowed path.  Holds ctx->mu for the build and synchronizes before the
// pointer is published, so concurrent cohort threads race to it safely.
static const G1Aff* msm_fixed_table(RngCtxImpl* ctx, uint32_t c) {
    const uint64_t N = ctx->srs_count;
    const uint32_t W = (256 + c - 1) / c;
    if (!ctx->srs_dev || N == 0 || c < 8 || c > 16) return nullptr;
    if ((uint64_t)W * N * sizeof(G1Aff) > (1ull << 30) || ((uint64_t)W * N >> 31))
        return nullptr;
    std::lock_guard<std::mutex> lk(ctx->mu);
    for (auto& t : ctx->fixed_tables)
        if (t.dev && t.c == c) return (const G1Aff*)t.dev;
    for (auto& t : ctx->fixed_tables) {
        if (t.dev) continue;
        void* dev = nullptr;
        if (hipMalloc(&dev, (uint64_t)W * N * sizeof(G1Aff)) != hipSuccess) return nullptr;
        hipLaunchKernelGGL(k_msm_fixed_table, dim3((uint32_t)((N + 255) / 256)), dim3(256),
                           0, RNG_STREAM, (const G1Aff*)ctx->srs_dev, (uint32_t)N, c, W,
                           (G1Aff*)dev);
        if (hipGetLastError() != hipSuccess ||
            hipStreamSynchronize(RNG_STREAM) != hipSuccess) {
            hipFree(dev);
            return nullptr;
        }
        t.c = c;
        t.dev = dev;
        return (const G1Aff*)dev;
    }
    return nullptr;
}

// ---- direct-lookup path over the SRS ----

static uint64_t msm_lookup_bytes(uint64_t N, uint32_t c) {
    return (((uint64_t)((256 + c - 1) / c) * N) << (c - 1)) * sizeof(G1Aff);
}

// Lookup table for window size c, built on first use from the window table
// of the same c.  The table must fit the byte budget (10 GiB unless
// RNG_MSM_LOOKUP_MAX_MB says otherwise: a policy, not a measurement) and half
// of the device memory free at that moment; nullptr otherwise, and after a
// failed allocation or build, and callers keep the bucket pipeline.  Holds
// ctx->mu for the build and synchronizes before the pointer is published.
static const G1Aff* msm_lookup_table(RngCtxImpl* ctx, uint32_t c) {
    const uint64_t N = ctx->srs_count;
    if (!ctx->srs_dev || N == 0 || c < MSM_LOOKUP_MIN_C || c > MSM_LOOKUP_MAX_C)
        return nullptr;
    const uint64_t bytes = msm_lookup_bytes(N, c);
    const int max_mb = msm_env().lookup_max_mb;
    if (max_mb <= 0 || bytes > ((uint64_t)max_mb << 20) || N >> 32) return nullptr;
    RngCtxImpl::LookupTable& t = ctx->lookup_tables[c - MSM_LOOKUP_MIN_C];
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (t.dev || t.tried) return (const G1Aff*)t.dev;
    }
    const G1Aff* fixed = msm_fixed_table(ctx, c);  // takes ctx->mu itself
    if (!fixed) return nullptr;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (t.dev || t.tried) return (const G1Aff*)t.dev;
    t.tried = true;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || bytes > free_b / 2) return nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    void* dev = nullptr;
    if (hipMalloc(&dev, bytes) != hipSuccess) {
        (void)hipGetLastError();  // out of memory is not an error here
        return nullptr;
    }
    const uint64_t rows = (uint64_t)((256 + c - 1) / c) * N;
    hipLaunchKernelGGL(k_msm_lookup_table, dim3((uint32_t)((rows + 255) / 256)), dim3(256), 0,
                       RNG_STREAM, fixed, rows, c, (G1Aff*)dev);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(RNG_STREAM) != hipSuccess) {
        hipFree(dev);
        return nullptr;
    }
    if (msm_env().debug)
        fprintf(stderr, "[msm] lookup table c=%u rows=%lu bytes=%lu build_ms=%.1f\n", c,
                (unsigned long)rows, (unsigned long)bytes,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0)
                    .count());
    t.dev = dev;
    return (const G1Aff*)dev;
}

// Where RNG_MSM_LOOKUP is unset: the paths on which the lookup sum replaces
// the bucket pipeline, as the A/B of profiles/msm_lookup_ab.json decided.
// Cohort = the fused rounds of a batch (B >= 16, as in msm_fixed_c); small =
// single proofs, preprocessing, link proofs.
constexpr bool MSM_LOOKUP_COHORT_DEFAULT = true;
constexpr bool MSM_LOOKUP_SMALL_DEFAULT = true;

static bool msm_lookup_wanted(uint32_t B) {
    const int sw = msm_env().lookup;
    if (sw >= 0) return sw != 0;
    return B >= 16 ? MSM_LOOKUP_COHORT_DEFAULT : MSM_LOOKUP_SMALL_DEFAULT;
}

// The selector: the largest c in {8, 9, 10} whose table fits (fewest adds
// per scalar), or RNG_MSM_LOOKUP_C alone.  *c_out = 0 where none does.
static const G1Aff* msm_lookup_select(RngCtxImpl* ctx, uint32_t* c_out) {
    const int c_env = msm_env().lookup_c;
    uint32_t lo = MSM_LOOKUP_MIN_C, hi = MSM_LOOKUP_MAX_C;
    if (c_env >= (int)lo && c_env <= (int)hi) lo = hi = (uint32_t)c_env;
    for (uint32_t c = hi; c >= lo; --c)
        if (const G1Aff* t = msm_lookup_table(ctx, c)) {
            *c_out = c;
            return t;
        }
    *c_out = 0;
    return nullptr;
}

// Scalars per lane: 1 until the batch is large, then as many (<= 8) as keep
// MSM_LOOKUP_MIN_LANES lanes.  256 CUs x 4 SIMDs x 3 waves x 64 = 196608
// lanes are resident at the kernel's occupancy, and a grid below that leaves
// wave slots empty; the headline sweep has 1 and 2 scalars per
// lane level, 4 behind by 1.6 % and 8 by 13 %.
constexpr uint64_t MSM_LOOKUP_MIN_LANES = 1ull << 18;
static uint32_t msm_lookup_per_lane(uint64_t m, uint32_t B) {
    const int l_env = msm_env().lookup_l;
    if (l_env >= 1 && l_env <= 8) return (uint32_t)l_env;
    uint32_t L = 1;
    while (L < 8 && m * B / (2 * L) >= MSM_LOOKUP_MIN_LANES) L *= 2;
    return L;
}

// block partials of the calling thread's lookup sums; a thread that only
// ever takes this path allocates nothing else
struct MsmLookupScratch {
    G1Jac* partials = nullptr;
    uint64_t cap = 0;
    ~MsmLookupScratch() { hip_free_guarded(partials); }
};
static thread_local MsmLookupScratch tls_msm_lookup;

// B polys of m canonical scalars (device) as plain signed sums of looked-up
// points: ONE kernel, one D2H copy of the block partials, one synchronize.
static int msm_lookup_run(const G1Aff* table, uint64_t N, const uint64_t* d_canon, uint64_t m,
                          uint32_t c, G1Jac* h_result, uint32_t B,
                          hipStream_t stream = RNG_STREAM) {
    const uint32_t W = (256 + c - 1) / c;
    const uint32_t L = msm_lookup_per_lane(m, B);
    const uint32_t bpp = (uint32_t)((m + 256ull * L - 1) / (256ull * L));
    const uint64_t np = (uint64_t)B * bpp;
    MsmLookupScratch& s = tls_msm_lookup;
    if (s.cap < np) {
        hipFree(s.partials);
        s.partials = nullptr;
        s.cap = 0;
        HIP_CHECK(hipMalloc(&s.partials, (np + np / 2 + 64) * sizeof(G1Jac)));
        s.cap = np + np / 2 + 64;
    }
    if (msm_env().debug)
        fprintf(stderr, "[msm] n=%lu B=%u lookup c=%u L=%u blocks=%u\n", (unsigned long)m, B, c,
                L, bpp);
    EvtTimer et;
    et.mark(stream);
    hipLaunchKernelGGL(k_msm_lookup_sum, dim3(bpp, B), dim3(256), 0, stream, d_canon,
                       (uint32_t)m, c, W, (uint32_t)N, L, table, s.partials);
    HIP_CHECK(hipGetLastError());
    et.mark(stream);
    std::vector<G1Jac> wsums((size_t)np);
    HIP_CHECK(hipMemcpyAsync(wsums.data(), s.partials, np * sizeof(G1Jac),
                             hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    // the whole sum reports as the bucket-reduce stage of tls_msm_times
    double ms = 0;
    et.collect(&ms, 1);
    for (double& t : tls_msm_times) t = 0;
    tls_msm_times[2] = ms;
    MsmShape sh{};  // what msm_host_fold reads: B groups of bpp partials, no windows
    sh.B = sh.G = B;
    sh.W = 1;
    sh.subb = bpp;
    sh.c = c;
    msm_host_fold(sh, wsums, h_result);
    return RNG_OK;
}

// Every SRS commitment goes through here: B polys of m canonical scalars
// each (device) against the first m SRS points.  window_c 0 = auto (the
// RNG_MSM_C tuning override applies); mode 0 = the lookup sum where
// msm_lookup_wanted and a table fits, else fixed-base where a table is
// allowed, else windowed; 1 = fixed-base (bucket pipeline) or error;
// 2 = windowed; 3 = lookup sum or error.
static int msm_srs_run(RngCtxImpl* ctx, const uint64_t* d_canon, uint64_t m, uint32_t B,
                       G1Jac* res, int window_c = 0, int mode = 0) {
    if (m == 0 || m > ctx->srs_count || B == 0) return RNG_ERR_BAD_ARG;
    const int c_env = msm_env().c;
    if (window_c == 0 && c_env >= 8 && c_env <= 16) window_c = c_env;
    if (window_c != 0 && (window_c < 8 || window_c > 16)) return RNG_ERR_BAD_ARG;
    if (mode == 3 || (mode == 0 && msm_fixed_enabled() && msm_lookup_wanted(B))) {
        uint32_t c = (uint32_t)window_c;
        const G1Aff* table = nullptr;
        if (B <= 65535)  // poly = blockIdx.y
            table = window_c ? msm_lookup_table(ctx, c) : msm_lookup_select(ctx, &c);
        if (table) return msm_lookup_run(table, ctx->srs_count, d_canon, m, c, res, B);
        if (mode == 3) return RNG_ERR_BAD_ARG;
    }
    if (mode == 1 || (mode == 0 && msm_fixed_enabled())) {
        uint32_t c = window_c ? (uint32_t)window_c : msm_fixed_c(m, B);
        uint32_t gb = 1;
        while ((1u << gb) <= B) ++gb;
        const G1Aff* table = (c + gb <= 32) ? msm_fixed_table(ctx, c) : nullptr;
        if (table)
            return msm_dev_run(MsmBases::table(table, ctx->srs_count), d_canon, m, c, res,
                               B);
        if (mode == 1) return RNG_ERR_BAD_ARG;
    }
    uint32_t c = window_c ? (uint32_t)window_c : msm_auto_c(m);
    if ((uint64_t)B * ((256 + c - 1) / c) > 60000) return RNG_ERR_BAD_ARG;  // g<<16 cap
    return msm_dev_run(MsmBases::plain((const G1Aff*)ctx->srs_dev), d_canon, m, c, res, B);
}

// ---- Lagrange-basis commitments of evaluation vectors ----

// internal status: this domain has no Lagrange bases (a base at infinity,
// n + 2 > srs_count, no table slot or memory); the prover falls back to the
// coefficient path, the test hook reports RNG_ERR_BAD_ARG
constexpr int MSM_LAGRANGE_UNUSABLE = -100;

// bases for domain size n; called with ctx->mu held
static int lagrange_build_bases(RngCtxImpl* ctx, uint64_t n, void** out_bases) {
    const uint32_t N = (uint32_t)n + 2;
    uint32_t logn = 0;
    while ((1ull << logn) < n) ++logn;
    const hipStream_t st = RNG_STREAM;
    G1Jac *pts = nullptr, *fin = nullptr;
    Fr* tw = nullptr;
    uint32_t* bad = nullptr;
    void* bases = nullptr;
    auto cleanup = [&] {
        hipFree(pts);
        hipFree(fin);
        hipFree(tw);
        hipFree(bad);
    };
    if (hipMalloc(&pts, n * sizeof(G1Jac)) != hipSuccess ||
        hipMalloc(&fin, (uint64_t)N * sizeof(G1Jac)) != hipSuccess ||
        hipMalloc(&tw, (n / 2) * sizeof(Fr)) != hipSuccess ||
        hipMalloc(&bad, 4) != hipSuccess ||
        hipMalloc(&bases, (uint64_t)N * sizeof(G1Aff)) != hipSuccess) {
        cleanup();
        hipFree(bases);
        return RNG_ERR_HIP;
    }
    const Fr winv = h_fr_root_of_unity((uint32_t)n).inverse();
    Fr nfr = Fr::one();
    for (uint32_t i = 0; i < logn; ++i) nfr = nfr.add(nfr);  // n = 2^logn
    Canon4 ninv;
    nfr.inverse().to_canonical(ninv.l);
    const G1Aff* srs = (const G1Aff*)ctx->srs_dev;
    hipMemsetAsync(bad, 0, 4, st);
    hipLaunchKernelGGL(k_pow_table, dim3((uint32_t)((n / 2 + 255) / 256)), dim3(256), 0, st,
                       tw, winv, (uint64_t)1, n / 2);
    hipLaunchKernelGGL(k_g1_ntt_load, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st,
                       srs, (uint32_t)n, pts);
    for (uint32_t h = (uint32_t)n / 2; h >= 1; h >>= 1)
        hipLaunchKernelGGL(k_g1_ntt_pass, dim3((uint32_t)((n / 2 + 63) / 64)), dim3(64), 0,
                           st, pts, (uint32_t)n, h, (const Fr*)tw);
    hipLaunchKernelGGL(k_g1_ntt_finish, dim3((N + 63) / 64), dim3(64), 0, st,
                       (const G1Jac*)pts, srs, (uint32_t)n, logn, ninv, fin);
    const uint32_t norm_threads = (N + LAG_NORM - 1) / LAG_NORM;
    hipLaunchKernelGGL(k_g1_normalize, dim3((norm_threads + 63) / 64), dim3(64), 0, st,
                       (const G1Jac*)fin, N, (G1Aff*)bases, bad);
    uint32_t h_bad = 1;
    bool ok = hipGetLastError() == hipSuccess &&
              hipMemcpyAsync(&h_bad, bad, 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
              hipStreamSynchronize(st) == hipSuccess;
    cleanup();
    if (!ok || h_bad) {
        hipFree(bases);
        return ok ? MSM_LAGRANGE_UNUSABLE : RNG_ERR_HIP;
    }
    *out_bases = bases;
    return RNG_OK;
}

// Window table over the Lagrange bases of domain n for window size c, both
// built on first use.  nullptr = unusable (callers fall back).  Holds
// ctx->mu for the builds and synchronizes before anything is published, as
// msm_fixed_table does, so concurrent threads race to it safely.
static const G1Aff* msm_lagrange_table(RngCtxImpl* ctx, uint64_t n, uint32_t c) {
    if (!ctx->srs_dev || n < 2 || (n & (n - 1)) || n > (1ull << 28) ||
        n + 2 > ctx->srs_count || c < 8 || c > 16)
        return nullptr;
    const uint64_t N = n + 2;
    const uint32_t W = (256 + c - 1) / c;
    if ((uint64_t)W * N * sizeof(G1Aff) > (1ull << 30)) return nullptr;
    static const int trace = msm_env().debug;
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto it = ctx->lagrange.find(n);
    if (it == ctx->lagrange.end()) {
        auto t0 = std::chrono::steady_clock::now();
        RngCtxImpl::LagrangeDomain dom;
        dom.usable = lagrange_build_bases(ctx, n, &dom.bases) == RNG_OK;
        it = ctx->lagrange.emplace(n, dom).first;
        if (trace)
            fprintf(stderr, "[lagrange] n=%lu bases %s in %.2f ms\n", (unsigned long)n,
                    dom.usable ? "built" : "UNUSABLE",
                    std::chrono::duration<double, std::milli>(
                        std::chrono::steady_clock::now() - t0).count());
    }
    RngCtxImpl::LagrangeDomain& dom = it->second;
    if (!dom.usable) return nullptr;
    for (auto& t : dom.tables)
        if (t.dev && t.c == c) return (const G1Aff*)t.dev;
    for (auto& t : dom.tables) {
        if (t.dev) continue;
        auto t0 = std::chrono::steady_clock::now();
        void* dev = nullptr;
        if (hipMalloc(&dev, (uint64_t)W * N * sizeof(G1Aff)) != hipSuccess) return nullptr;
        hipLaunchKernelGGL(k_msm_fixed_table, dim3((uint32_t)((N + 255) / 256)), dim3(256),
                           0, RNG_STREAM, (const G1Aff*)dom.bases, (uint32_t)N, c, W,
                           (G1Aff*)dev);
        if (hipGetLastError() != hipSuccess ||
            hipStreamSynchronize(RNG_STREAM) != hipSuccess) {
            hipFree(dev);
            return nullptr;
        }
        t.c = c;
        t.dev = dev;
        if (trace)
            fprintf(stderr, "[lagrange] n=%lu c=%u table (%.1f MB) in %.2f ms\n",
                    (unsigned long)n, c, (double)W * N * sizeof(G1Aff) / 1e6,
                    std::chrono::duration<double, std::milli>(
                        std::chrono::steady_clock::now() - t0).count());
        return (const G1Aff*)dev;
    }
    return nullptr;
}

// Window size on the Lagrange path.  The density figure is the share of
// non-zero scalars, which does not depend on c.  Sparse witnesses (the
// settlement circuit: ~19 % non-zero values, most of them one digit long)
// leave so few entries that aggregation over B*2^(c-1) buckets is all that
// remains, so they take the smallest table-backed window (c = 8 beat 10 and
// 13 at the settlement cohort shape: DESIGN §4.1).  A dense witness (more
// than half of the scalars non-zero; the validity circuits are at 86-96 %)
// gains nothing here: 0 tells the prover to commit the coefficients as
// before, so such a domain never builds bases or tables.  The 1/2 threshold
// is reasoned, not tuned: the circuits sit at 19 % and at 86 % and above.
// The test hook commits dense input at MSM_LAGRANGE_DENSE_C whatever B is,
// so a domain sees at most two window sizes.
constexpr uint32_t MSM_LAGRANGE_SPARSE_C = 8, MSM_LAGRANGE_DENSE_C = 13;
static uint32_t msm_lagrange_c(uint64_t n, uint32_t B, uint64_t nonzero) {
    return nonzero * 2 <= (uint64_t)B * n ? MSM_LAGRANGE_SPARSE_C : 0;
}

// ---- lookup sum over compacted entries ----
// After compaction a sparse batch is a few thousand entries per poly, already
// grouped by poly, so with every digit multiple of every base precomputed the
// commitment is a plain signed sum: no sort, buckets, merge or combine.

// RNG_R1_LOOKUP unset: as the A/B of profiles/lagrange_lookup_ab.json decided
constexpr bool R1_LOOKUP_DEFAULT = true;

static bool r1_lookup_wanted(uint32_t B) {
    const int sw = msm_env().r1_lookup;
    return msm_lookup_wanted(B) && (sw < 0 ? R1_LOOKUP_DEFAULT : sw == 1);
}

// Lookup table over the bases of domain n for window size c, built on first
// use from the domain's window table of the same c.  Budget, free-memory rule
// and `tried` as in msm_lookup_table; a row count that would reach the sign
// bit of an entry gets no table.  Holds ctx->mu for the build and
// synchronizes before the pointer is published.
static const G1Aff* msm_lagrange_lookup_table(RngCtxImpl* ctx, uint64_t n, uint32_t c) {
    if (c < MSM_LOOKUP_MIN_C || c > MSM_LOOKUP_MAX_C) return nullptr;
    const uint64_t N = n + 2;
    const uint64_t bytes = msm_lookup_bytes(N, c);
    const int max_mb = msm_env().lookup_max_mb;
    if (max_mb <= 0 || bytes > ((uint64_t)max_mb << 20) || !msm_entry_rows_fit(N, c))
        return nullptr;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        auto it = ctx->lagrange.find(n);
        if (it != ctx->lagrange.end()) {
            RngCtxImpl::LookupTable& t = it->second.lookup[c - MSM_LOOKUP_MIN_C];
            if (t.dev || t.tried || !it->second.usable) return (const G1Aff*)t.dev;
        }
    }
    const G1Aff* fixed = msm_lagrange_table(ctx, n, c);  // takes ctx->mu itself
    if (!fixed) return nullptr;
    std::lock_guard<std::mutex> lk(ctx->mu);
    RngCtxImpl::LookupTable& t = ctx->lagrange.find(n)->second.lookup[c - MSM_LOOKUP_MIN_C];
    if (t.dev || t.tried) return (const G1Aff*)t.dev;
    t.tried = true;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || bytes > free_b / 2) return nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    void* dev = nullptr;
    if (hipMalloc(&dev, bytes) != hipSuccess) {
        (void)hipGetLastError();  // out of memory is not an error here
        return nullptr;
    }
    const uint64_t rows = msm_table_rows(N, c);
    hipLaunchKernelGGL(k_msm_lookup_table, dim3((uint32_t)((rows + 255) / 256)), dim3(256), 0,
                       RNG_STREAM, fixed, rows, c, (G1Aff*)dev);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(RNG_STREAM) != hipSuccess) {
        hipFree(dev);
        return nullptr;
    }
    if (msm_env().debug)
        fprintf(stderr,
                "[msm] lagrange lookup table n=%lu c=%u rows=%lu bytes=%lu build_ms=%.1f\n",
                (unsigned long)n, c, (unsigned long)rows, (unsigned long)bytes,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0)
                    .count());
    t.dev = dev;
    return (const G1Aff*)dev;
}

// The calling thread's buffers for the sum over compacted entries; every
// dimension grows with slack and never shrinks, so a thread that alternates
// this path with the dense lookup sum allocates nothing per proof.
struct R1LookupScratch {
    uint32_t *counts = nullptr, *offs = nullptr;  // cap_scalars + 2 words each
    uint64_t cap_scalars = 0;
    void* scan_temp = nullptr;
    size_t scan_temp_bytes = 0;
    uint32_t *keys = nullptr, *vals = nullptr;
    uint64_t cap_entries = 0;
    G1Jac* partials = nullptr;
    uint64_t cap_partials = 0;
    ~R1LookupScratch() {
        for (void* b : {(void*)counts, (void*)offs, scan_temp, (void*)keys, (void*)vals,
                        (void*)partials})
            hip_free_guarded(b);
    }
};
static thread_local R1LookupScratch tls_r1_lookup;

// grow `*buf` to hold `want` elements of `elem` bytes (contents are not kept)
static int r1_scratch_grow(void** buf, uint64_t* cap, uint64_t want, size_t elem) {
    if (*cap >= want) return RNG_OK;
    hipFree(*buf);
    *buf = nullptr;
    *cap = 0;
    const uint64_t ncap = want + want / 2 + 64;
    HIP_CHECK(hipMalloc(buf, ncap * elem));
    *cap = ncap;
    return RNG_OK;
}

// Blocks per poly: about R1_LOOKUP_PER_LANE entries per lane at the batch's
// mean entry count.  A lane's chain is its madds plus the block's 8 fold
// levels, so a few entries per lane keep both short while the partials the
// host folds stay few (settlement cohort: ~2.2 k entries per poly -> S = 3).
constexpr uint32_t R1_LOOKUP_PER_LANE = 4, R1_LOOKUP_MAX_S = 64;
static uint32_t r1_lookup_blocks(uint64_t entries, uint32_t B) {
    const int s_env = msm_env().r1_lookup_s;
    if (s_env >= 1 && s_env <= (int)R1_LOOKUP_MAX_S) return (uint32_t)s_env;
    const uint64_t per_block = 256ull * R1_LOOKUP_PER_LANE;
    uint64_t S = (entries / B + per_block - 1) / per_block;
    return (uint32_t)(S < 1 ? 1 : S > R1_LOOKUP_MAX_S ? R1_LOOKUP_MAX_S : S);
}

// internal results of r1_lookup_run: the gate found the batch dense (nothing
// was committed); the domain has no lookup table (the caller keeps the
// bucket pipeline)
constexpr int R1_LOOKUP_DENSE = -101, R1_LOOKUP_NO_TABLE = -102;

// B blocks of n + 2 canonical scalars as a sum of looked-up points over the
// compacted entries at window size c.  Two synchronizes: (1) digit count (+
// the density figure where `gate`) and scan, read back as {entry total,
// non-zero scalars}; (2) compact, sum, the S partials per poly.
static int r1_lookup_run(RngCtxImpl* ctx, uint64_t n, const uint64_t* d_canon, uint32_t B,
                         uint32_t c, bool gate, G1Jac* h_result) {
    const hipStream_t stream = RNG_STREAM;
    const uint32_t N = (uint32_t)n + 2, W = (256 + c - 1) / c;
    const uint32_t ns = B * N;
    {  // a domain that was refused its table stays on the bucket path
        std::lock_guard<std::mutex> lk(ctx->mu);
        auto it = ctx->lagrange.find(n);
        if (it != ctx->lagrange.end()) {
            const RngCtxImpl::LookupTable& t = it->second.lookup[c - MSM_LOOKUP_MIN_C];
            if (!it->second.usable || (t.tried && !t.dev)) return R1_LOOKUP_NO_TABLE;
        }
    }
    R1LookupScratch& s = tls_r1_lookup;
    if (s.cap_scalars < ns) {
        uint64_t cap_c = s.cap_scalars, cap_o = s.cap_scalars;
        int rc = r1_scratch_grow((void**)&s.counts, &cap_c, (uint64_t)ns + 2, 4);
        if (rc == RNG_OK) rc = r1_scratch_grow((void**)&s.offs, &cap_o, (uint64_t)ns + 2, 4);
        s.cap_scalars = 0;
        if (rc != RNG_OK) return rc;
        hipFree(s.scan_temp);
        s.scan_temp = nullptr;
        (void)rocprim::exclusive_scan(nullptr, s.scan_temp_bytes, s.counts, s.offs, 0u, cap_c,
                                      rocprim::plus<uint32_t>(), stream);
        HIP_CHECK(hipMalloc(&s.scan_temp, s.scan_temp_bytes));
        s.cap_scalars = cap_c - 2;
    }
    // offs[0 .. ns]: entry offsets, offs[ns] the total; offs[ns + 1]: the
    // non-zero scalar count, so one 8-byte copy reads both
    EvtTimer et;
    et.mark(stream);
    HIP_CHECK(hipMemsetAsync(s.offs + ns + 1, 0, 4, stream));
    hipLaunchKernelGGL(k_msm_digit_count_density, dim3(ns / 256 + 1), dim3(256), 0, stream,
                       d_canon, ns, c, W, s.counts, s.offs + ns + 1);
    HIP_CHECK(hipGetLastError());
    (void)rocprim::exclusive_scan(s.scan_temp, s.scan_temp_bytes, s.counts, s.offs, 0u,
                                  (size_t)ns + 1, rocprim::plus<uint32_t>(), stream);
    et.mark(stream);
    uint32_t back[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(back, s.offs + ns, 8, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    const uint64_t entries = back[0];
    if (gate && msm_lagrange_c(n, B, back[1]) == 0) return R1_LOOKUP_DENSE;
    const G1Aff* table = msm_lagrange_lookup_table(ctx, n, c);
    if (!table) return R1_LOOKUP_NO_TABLE;
    const uint32_t S = r1_lookup_blocks(entries, B);
    if (msm_env().debug)
        fprintf(stderr, "[msm] n=%lu B=%u entry-lookup c=%u S=%u entries=%lu (compacted)\n",
                (unsigned long)N, B, c, S, (unsigned long)entries);
    for (double& t : tls_msm_times) t = 0;
    if (entries == 0) {  // every scalar zero
        for (uint32_t b = 0; b < B; ++b) h_result[b] = G1Jac::identity();
        et.collect(tls_msm_times, 1);
        return RNG_OK;
    }
    const uint64_t np = (uint64_t)B * S;
    int rc = r1_scratch_grow((void**)&s.partials, &s.cap_partials, np, sizeof(G1Jac));
    if (rc != RNG_OK) return rc;
    if (s.cap_entries < entries) {
        uint64_t cap_k = s.cap_entries, cap_v = s.cap_entries;
        rc = r1_scratch_grow((void**)&s.keys, &cap_k, entries, 4);
        if (rc == RNG_OK) rc = r1_scratch_grow((void**)&s.vals, &cap_v, entries, 4);
        s.cap_entries = rc == RNG_OK ? cap_k : 0;
        if (rc != RNG_OK) return rc;
    }
    et.mark(stream);
    hipLaunchKernelGGL(k_msm_digits_compact, dim3((ns + 255) / 256), dim3(256), 0, stream,
                       d_canon, N, c, W, B, N, s.offs, s.keys, s.vals);
    HIP_CHECK(hipGetLastError());
    et.mark(stream);
    hipLaunchKernelGGL(k_msm_entry_lookup_sum, dim3(S, B), dim3(256), 0, stream, s.keys,
                       s.vals, s.offs, N, c, table, s.partials);
    HIP_CHECK(hipGetLastError());
    et.mark(stream);
    std::vector<G1Jac> wsums((size_t)np);
    HIP_CHECK(hipMemcpyAsync(wsums.data(), s.partials, np * sizeof(G1Jac),
                             hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    // digits = count + scan + compact; the sum reports as the bucket-reduce
    // stage, as msm_lookup_run's does
    double ms[4] = {0, 0, 0, 0};  // count+scan, the read-back gap, compact, sum
    et.collect(ms, 4);
    tls_msm_times[0] = ms[0] + ms[2];
    tls_msm_times[2] = ms[3];
    MsmShape sh{};  // what msm_host_fold reads: B groups of S partials, no windows
    sh.B = sh.G = B;
    sh.W = 1;
    sh.subb = S;
    sh.c = c;
    msm_host_fold(sh, wsums, h_result);
    return RNG_OK;
}

// B evaluation vectors committed against the Lagrange bases of domain n:
// d_canon holds B blocks of n + 2 canonical scalars (n evaluations, then the
// poly's two blinders).  Same group elements as msm_srs_run over the blinded
// coefficients.  window_c 0 = msm_lagrange_c (RNG_MSM_C overrides); where
// that declines a dense batch the result is MSM_LAGRANGE_UNUSABLE, unless
// dense_too (the test hook) asks for the commitment anyway.  Where the window
// is in the lookup range and the domain has a lookup table the commitment is
// r1_lookup_run's sum over compacted entries (two synchronizes); otherwise
// the bucket pipeline over compacted digits, as before.
static int msm_lagrange_run(RngCtxImpl* ctx, uint64_t n, const uint64_t* d_canon, uint32_t B,
                            G1Jac* res, int window_c = 0, bool dense_too = false) {
    if (n < 2 || (n & (n - 1)) || B == 0 || !d_canon) return RNG_ERR_BAD_ARG;
    if (n + 2 > ctx->srs_count) return MSM_LAGRANGE_UNUSABLE;
    const int c_env = msm_env().c;
    if (window_c == 0 && c_env >= 8 && c_env <= 16) window_c = c_env;
    if (window_c != 0 && (window_c < 8 || window_c > 16)) return RNG_ERR_BAD_ARG;
    uint32_t c = (uint32_t)window_c;
    // the lookup sum over compacted entries, where the window the batch would
    // get has a lookup table: the density gate rides on its digit count
    const uint32_t c_try = c ? c : MSM_LAGRANGE_SPARSE_C;
    if (r1_lookup_wanted(B) && c_try >= MSM_LOOKUP_MIN_C && c_try <= MSM_LOOKUP_MAX_C &&
        B <= 65535 && msm_table_rows(n + 2, c_try) * B < (1ull << 32)) {
        int rc = r1_lookup_run(ctx, n, d_canon, B, c_try, /*gate=*/c == 0, res);
        if (rc != R1_LOOKUP_DENSE && rc != R1_LOOKUP_NO_TABLE) return rc;
        if (rc == R1_LOOKUP_DENSE) {
            if (!dense_too) return MSM_LAGRANGE_UNUSABLE;
            c = MSM_LAGRANGE_DENSE_C;
        } else {
            c = c_try;  // sparse (or the caller's c), but no table: the buckets
        }
    }
    if (c == 0) {
        MsmScratch* s = nullptr;
        // any shape sizes the scratch; head_count doubles as the counter
        int rc = msm_scratch_ensure(msm_shape(n + 2, B, 8, true, true), RNG_STREAM, &s);
        if (rc != RNG_OK) return rc;
        const uint32_t ns = (uint32_t)(B * (n + 2));
        uint32_t nz = 0;
        HIP_CHECK(hipMemsetAsync(s->head_count, 0, 4, RNG_STREAM));
        hipLaunchKernelGGL(k_count_nonzero_scalars, dim3((ns + 255) / 256), dim3(256), 0,
                           RNG_STREAM, d_canon, ns, s->head_count);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(&nz, s->head_count, 4, hipMemcpyDeviceToHost, RNG_STREAM));
        HIP_CHECK(hipStreamSynchronize(RNG_STREAM));
        c = msm_lagrange_c(n, B, nz);
        if (c == 0) {
            if (!dense_too) return MSM_LAGRANGE_UNUSABLE;
            c = MSM_LAGRANGE_DENSE_C;
        }
    }
    uint32_t gb = 1;
    while ((1u << gb) <= B) ++gb;
    if (c + gb > 32) return MSM_LAGRANGE_UNUSABLE;
    const G1Aff* table = msm_lagrange_table(ctx, n, c);
    if (!table) return MSM_LAGRANGE_UNUSABLE;
    return msm_dev_run(MsmBases::table(table, n + 2), d_canon, n + 2, c, res, B, RNG_STREAM,
                       true);
}

// RNG_R1_LAGRANGE (ProverEnv::r1_lagrange): 0 = round 1 commits the blinded
// coefficients, 1 = commits the evaluations against the Lagrange bases, for
// every k.  Unset: on from this cohort size up.  One proof (B = 5) measured
// no gain and its first prove pays the bases build (DESIGN §4.1, table row
// `--jobs 1`; profiles/lagrange_commit_ab.json); cohorts gain.
constexpr uint32_t R1_LAGRANGE_MIN_K = 2;

// ---------------- TurboPlonk prover (GPU) ----------------

static int ensure_coset_tables(RngCtxImpl* ctx, NttPlan* p) {
    std::lock_guard<std::mutex> lk(ctx->mu);  // thread-safe lazy build
    if (p->gpow) return RNG_OK;
    uint32_t m = p->n;
    Fr g = Fr::from_u64(FR_GENERATOR);
    Fr gi = g.inverse();
    if (build_pow_table(&p->gpow, g, 1, m) != RNG_OK) return RNG_ERR_HIP;
    if (build_pow_table(&p->gpow_inv, gi, 1, m) != RNG_OK) return RNG_ERR_HIP;
    Fr wm = h_fr_root_of_unity(m);
    if (build_pow_table(&p->xpow, wm, 1, m) != RNG_OK) return RNG_ERR_HIP;
    uint32_t blocks = (m + 255) / 256;
    hipLaunchKernelGGL(k_scale_const, dim3(blocks), dim3(256), 0, 0, p->xpow, g, m);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    return RNG_OK;
}

// forward coset NTT of device buffer `in` (m elements, coefficient form),
// result into `out` (in is clobbered)
static int coset_fwd_dev(RngCtxImpl* ctx, Fr* in, Fr* out, uint32_t m) {
    NttPlan* p = get_plan(ctx, m, 1);
    if (!p) return RNG_ERR_HIP;
    if (ensure_coset_tables(ctx, p) != RNG_OK) return RNG_ERR_HIP;
    uint32_t blocks = (m + 255) / 256;
    hipLaunchKernelGGL(k_mul_pointwise, dim3(blocks), dim3(256), 0, RNG_STREAM, in,
                       p->gpow, m);
    HIP_CHECK(hipGetLastError());
    return ntt_dev_run(ctx, in, out, m, 1, false, RNG_STREAM);
}

// per-thread device scratch of preprocessing and link proofs at size n (the
// prover has its own, CohortScratch)
struct ProveScratch {
    static constexpr uint32_t SLOTS = 13;  // one fused commit: the 13 selectors
    uint64_t n = 0;
    Fr* tmp = nullptr;       // 8n: padded input of one coset transform
    Fr* stage = nullptr;     // SLOTS x (n+3) coefficient staging
    uint64_t* canon = nullptr;  // SLOTS x 4*(n+3) canonical scalars for commits
    ~ProveScratch() {
        for (void* b : {(void*)tmp, (void*)stage, (void*)canon}) hip_free_guarded(b);
    }
};

struct PlonkPkImpl : PlonkPkHost {  // host half: plonk_rounds.hpp
    Fr* sel_coset = nullptr;   // device 13*m
    Fr* sig_coset = nullptr;   // device 5*m
    Fr* l1_coset = nullptr;    // device m
    Fr* sig_evals_dev = nullptr;  // device 5*n (grand-product stage)
    Fr* wpow_dev = nullptr;       // device n: w^t
    Fr* coef_dev = nullptr;       // device 18*n: selq[0..12], sigp[0..4] (R4 + R5 stage)
    RngCtxImpl* ctx = nullptr;
    ~PlonkPkImpl() {
        for (void* b : {(void*)sel_coset, (void*)sig_coset, (void*)l1_coset,
                        (void*)sig_evals_dev, (void*)wpow_dev, (void*)coef_dev})
            hip_free_guarded(b);
    }
};

static thread_local std::unique_ptr<ProveScratch> tls_prove_scratch;

static int prove_scratch_ensure(uint64_t n) {
    if (tls_prove_scratch && tls_prove_scratch->n >= n) return RNG_OK;
    tls_prove_scratch = std::make_unique<ProveScratch>();
    ProveScratch* s = tls_prove_scratch.get();
    HIP_CHECK(hipMalloc(&s->tmp, 8 * n * sizeof(Fr)));
    HIP_CHECK(hipMalloc(&s->stage, ProveScratch::SLOTS * (n + 3) * sizeof(Fr)));
    HIP_CHECK(hipMalloc(&s->canon, ProveScratch::SLOTS * 4 * (n + 3) * 8));
    s->n = n;
    return RNG_OK;
}

// ---------------- R2: permutation grand product ----------------

// RNG_Z_DEVICE (ProverEnv::z_device): 0 = host loops, 1 = device stage
// (perm_kernels.hip), for every k.  Unset: the default below, set by the
// A/B measurement in DESIGN.md §4.5.
constexpr bool Z_DEVICE_DEFAULT = true;

// host loop: n evaluations of one proof's z into ze
static void perm_product_host(const PlonkPkImpl& pk, const Fr& w, const Fr* wires,
                              const Fr& beta, const Fr& gamma, Fr* ze) {
    const uint64_t n = pk.n;
    std::vector<Fr> znum(n), zden(n);
    Fr wi = Fr::one();
    for (uint64_t i = 0; i < n; ++i) {
        Fr num = Fr::one(), den = Fr::one();
        for (int j = 0; j < 5; ++j) {
            Fr wv = wires[(size_t)j * n + i];
            num = num.mul(wv.add(beta.mul(pk.k[j]).mul(wi)).add(gamma));
            den = den.mul(wv.add(beta.mul(pk.sig_evals[j][i])).add(gamma));
        }
        znum[i] = num;
        zden[i] = den;
        wi = wi.mul(w);
    }
    std::vector<Fr> zden_inv = hbatch_inverse(zden);
    ze[0] = Fr::one();
    for (uint64_t i = 1; i < n; ++i) ze[i] = ze[i - 1].mul(znum[i - 1]).mul(zden_inv[i - 1]);
}

struct PermScratch {  // per-thread small buffers of the device stage (~2 MiB)
    Fr* dev = nullptr;       // one allocation, carved below
    Fr* tile_tot = nullptr;  // 2*PERM_MAX_BATCH * PERM_MAX_TILES
    Fr* tile_pre = nullptr;  // same
    Fr* totals = nullptr;    // 2*PERM_MAX_BATCH sequence totals (num, then den)
    Fr* qinv = nullptr;      // PERM_MAX_BATCH
    Fr* bg = nullptr;        // PERM_MAX_BATCH x (beta, gamma)
    std::vector<Fr> h_bg, h_q;  // host staging (outlives the async copies)
    ~PermScratch() { hip_free_guarded(dev); }
};

static thread_local std::unique_ptr<PermScratch> tls_perm_scratch;

static PermScratch* perm_scratch_get() {
    if (tls_perm_scratch) return tls_perm_scratch.get();
    auto s = std::make_unique<PermScratch>();
    const size_t tiles = (size_t)2 * PERM_MAX_BATCH * PERM_MAX_TILES;
    const size_t elems = 2 * tiles + 5 * (size_t)PERM_MAX_BATCH;
    if (hipMalloc(&s->dev, elems * sizeof(Fr)) != hipSuccess) return nullptr;
    s->tile_tot = s->dev;
    s->tile_pre = s->tile_tot + tiles;
    s->totals = s->tile_pre + tiles;
    s->qinv = s->totals + 2 * PERM_MAX_BATCH;
    s->bg = s->qinv + PERM_MAX_BATCH;
    s->h_bg.resize(2 * PERM_MAX_BATCH);
    s->h_q.resize(PERM_MAX_BATCH);
    tls_perm_scratch = std::move(s);
    return tls_perm_scratch.get();
}

// The device stage, on RNG_STREAM.  Device pointers: wires (batch x 5 x n),
// sigma (5 x n), wpow (n), nd (2*batch*n workspace: num/den terms, scanned in
// place), z (batch x n out; may not alias nd).  bg = batch x (beta, gamma) on
// the host.  One stream sync in the middle: the batch den totals come back,
// are inverted on the host (a Fermat chain is a ~380-deep dependent
// multiplication chain, tens of µs on a host core against an estimated
// millisecond on one GPU lane) and go up again.
static int perm_product_dev(const Fr* wires, const Fr* sigma, const Fr* wpow,
                            const Fr k5[5], const Fr* bg, uint64_t n64, uint64_t batch64,
                            Fr* nd, Fr* z) {
    if (n64 < 2 || (n64 & (n64 - 1)) || n64 > PERM_MAX_N || batch64 < 1 ||
        batch64 > PERM_MAX_BATCH)
        return RNG_ERR_BAD_ARG;
    const uint32_t n = (uint32_t)n64, batch = (uint32_t)batch64;
    PermScratch* ps = perm_scratch_get();
    if (!ps) return RNG_ERR_HIP;
    memcpy(ps->h_bg.data(), bg, 2 * (size_t)batch * sizeof(Fr));
    HIP_CHECK(hipMemcpyAsync(ps->bg, ps->h_bg.data(), 2 * (size_t)batch * sizeof(Fr),
                             hipMemcpyHostToDevice, RNG_STREAM));
    PermK5 kk;
    for (int j = 0; j < 5; ++j) kk.k[j] = k5[j];
    const uint32_t rows_blocks = (uint32_t)(((uint64_t)batch * n + 255) / 256);
    hipLaunchKernelGGL(k_perm_terms, dim3(rows_blocks), dim3(256), 0, RNG_STREAM, wires,
                       sigma, wpow, ps->bg, kk, nd, n, batch);
    HIP_CHECK(hipGetLastError());
    const uint32_t tiles = (n + PERM_TILE - 1) / PERM_TILE, nseq = 2 * batch;
    if (tiles == 1) {
        hipLaunchKernelGGL(k_perm_scan_apply<false>, dim3(nseq), dim3(PERM_WG), 0,
                           RNG_STREAM, nd, (const Fr*)nullptr, ps->totals, n, 1u, batch);
        HIP_CHECK(hipGetLastError());
    } else {
        hipLaunchKernelGGL(k_perm_tile_reduce, dim3(nseq * tiles), dim3(PERM_WG), 0,
                           RNG_STREAM, nd, ps->tile_tot, n, tiles, batch);
        HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_perm_tile_prefix, dim3(nseq), dim3(PERM_WG), 0, RNG_STREAM,
                           ps->tile_tot, ps->tile_pre, ps->totals, tiles);
        HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_perm_scan_apply<true>, dim3(nseq * tiles), dim3(PERM_WG), 0,
                           RNG_STREAM, nd, ps->tile_pre, ps->totals, n, tiles, batch);
        HIP_CHECK(hipGetLastError());
    }
    // Q^-1 per proof; a zero total inverts to zero (Fermat), and must not
    // zero the other proofs' inverses in the shared batch inversion
    HIP_CHECK(hipMemcpyAsync(ps->h_q.data(), ps->totals + batch, batch * sizeof(Fr),
                             hipMemcpyDeviceToHost, RNG_STREAM));
    HIP_CHECK(hipStreamSynchronize(RNG_STREAM));
    {
        std::vector<Fr> q(ps->h_q.begin(), ps->h_q.begin() + batch);
        for (auto& v : q)
            if (v.is_zero()) v = Fr::one();
        q = hbatch_inverse(q);
        for (uint32_t p = 0; p < batch; ++p)
            ps->h_q[p] = ps->h_q[p].is_zero() ? Fr::zero() : q[p];
    }
    HIP_CHECK(hipMemcpyAsync(ps->qinv, ps->h_q.data(), batch * sizeof(Fr),
                             hipMemcpyHostToDevice, RNG_STREAM));
    hipLaunchKernelGGL(k_perm_finalize, dim3(rows_blocks), dim3(256), 0, RNG_STREAM, nd,
                       ps->qinv, z, n, batch);
    HIP_CHECK(hipGetLastError());
    return RNG_OK;
}

// tail of a KZG commit: B polys of m Montgomery coefficients staged on the
// device -> canonical scalars -> ONE fused MSM over the SRS bases.  The
// callers turn the Jacobian results affine with jacs_to_affine.
static int commit_staged_jac(RngCtxImpl* ctx, const Fr* stage, uint64_t* canon, uint64_t m,
                             uint32_t B, G1Jac* res) {
    uint32_t blocks = (uint32_t)((B * m + 255) / 256);
    hipLaunchKernelGGL(k_fr_to_canonical, dim3(blocks), dim3(256), 0, RNG_STREAM, stage,
                       canon, (uint32_t)(B * m));
    HIP_CHECK(hipGetLastError());
    // window size: auto by problem size; RNG_MSM_C overrides for tuning
    return msm_srs_run(ctx, canon, m, B, res);
}

// B independent Jacobian results -> affine.  On the pool only from B = 8 up:
// the pool admits one job at a time and every job wakes all its workers, so
// the five-element jobs of concurrent single proofs would queue on each other.
static void jacs_to_affine(const G1Jac* res, uint32_t B, G1Aff* out, bool* out_inf) {
    auto one = [&](uint32_t b) { jac_to_affine(res[b], &out[b], &out_inf[b]); };
    if (B >= 8)
        HostPool::inst().parallel_for(B, one);
    else
        for (uint32_t b = 0; b < B; ++b) one(b);
}

// commit B polynomials ALREADY staged on the device in `stage` (B consecutive
// m-coefficient blocks, Montgomery form; `canon` holds 4 u64 per coefficient)
static int commit_staged(RngCtxImpl* ctx, const Fr* stage, uint64_t* canon, uint64_t m,
                         uint32_t B, G1Aff* out, bool* out_inf) {
    if (m > ctx->srs_count) return RNG_ERR_BAD_ARG;
    std::vector<G1Jac> res(B);
    int rc = commit_staged_jac(ctx, stage, canon, m, B, res.data());
    if (rc != RNG_OK) return rc;
    jacs_to_affine(res.data(), B, out, out_inf);
    return RNG_OK;
}

// commit to B host coefficient vectors via ONE fused GPU MSM over the SRS
// bases (shorter polys zero-padded to the longest; zero scalars cost
// nothing).  `stage` holds stage_elems coefficients, `canon` 4 u64 for each.
static int commit_host_polys(RngCtxImpl* ctx, const std::vector<Fr>* const* polys,
                             uint32_t B, Fr* stage, uint64_t* canon, uint64_t stage_elems,
                             G1Aff* out, bool* out_inf) {
    uint64_t m = 0;
    for (uint32_t b = 0; b < B; ++b)
        if (polys[b]->size() > m) m = polys[b]->size();
    if (m > ctx->srs_count || B * m > stage_elems) return RNG_ERR_BAD_ARG;
    // pack on the host and ship ONE H2D copy: B small async copies of
    // pageable memory each pay a staging round trip.  Plain local (NOT
    // thread_local): pool workers reference it from their own threads.
    std::vector<Fr> packed(B * m);
    auto pack = [&](uint32_t b) {
        memcpy(packed.data() + (size_t)b * m, polys[b]->data(),
               polys[b]->size() * sizeof(Fr));
        memset(packed.data() + (size_t)b * m + polys[b]->size(), 0,
               (m - polys[b]->size()) * sizeof(Fr));
    };
    if (B >= 8)
        HostPool::inst().parallel_for(B, pack);
    else
        for (uint32_t b = 0; b < B; ++b) pack(b);
    HIP_CHECK(hipMemcpyAsync(stage, packed.data(), B * m * sizeof(Fr), hipMemcpyHostToDevice,
                             RNG_STREAM));
    return commit_staged(ctx, stage, canon, m, B, out, out_inf);
}

// the same out of ProveScratch (preprocessing, link proofs): B <= SLOTS
// polynomials of at most n + 3 coefficients
static int commit_dev_batch(RngCtxImpl* ctx, const std::vector<Fr>* const* polys,
                            uint32_t B, G1Aff* out, bool* out_inf) {
    ProveScratch* s = tls_prove_scratch.get();
    return commit_host_polys(ctx, polys, B, s->stage, s->canon,
                             ProveScratch::SLOTS * (s->n + 3), out, out_inf);
}

static int commit_dev(RngCtxImpl* ctx, const std::vector<Fr>& coeffs, G1Aff* out,
                      bool* out_inf) {
    const std::vector<Fr>* p = &coeffs;
    return commit_dev_batch(ctx, &p, 1, out, out_inf);
}

// ---------------- R4 + R5: evaluations, linearization, openings ----------------

// RNG_OPEN_DEVICE (ProverEnv::open_device): 0 = the host rounds
// (rounds_4_5), 1 = the device stage (open_kernels.hip), for every k.
// Unset: the default below, set by the A/B measurement in DESIGN.md §4.5
// (profiles/open_device_ab.json).
constexpr bool OPEN_DEVICE_DEFAULT = true;
static_assert(OPEN_TERMS == OPEN_COUNT, "k_open_lincomb follows open_scalars");

// the ten evaluations of every proof of a full cohort, and any one call
constexpr size_t OPEN_MAX_EVALS = 10 * (size_t)OPEN_MAX_BATCH;
static_assert(OPEN_MAX_EVALS >= OPEN_MAX_SEQ, "one call's results fit");

struct OpenScratch {  // per-thread small buffers of the device stage (~2.7 MiB)
    Fr* dev = nullptr;      // one allocation, carved below
    Fr* tile_io = nullptr;  // OPEN_MAX_SEQ * OPEN_MAX_TILES tile totals / carries
    Fr* pts = nullptr;      // OPEN_MAX_SEQ points (the prover: k x (zeta, zeta*w))
    Fr* evals = nullptr;    // OPEN_MAX_EVALS reduce-mode results
    Fr* scal = nullptr;     // OPEN_MAX_BATCH x 29 scalars
    std::vector<Fr> h_up, h_evals;  // host staging (outlives the async copies)
    ~OpenScratch() { hip_free_guarded(dev); }
};

static thread_local std::unique_ptr<OpenScratch> tls_open_scratch;

static OpenScratch* open_scratch_get() {
    if (tls_open_scratch) return tls_open_scratch.get();
    auto s = std::make_unique<OpenScratch>();
    const size_t tiles = (size_t)OPEN_MAX_SEQ * OPEN_MAX_TILES;
    const size_t elems =
        tiles + OPEN_MAX_SEQ + OPEN_MAX_EVALS + (size_t)OPEN_MAX_BATCH * OPEN_TERMS;
    if (hipMalloc(&s->dev, elems * sizeof(Fr)) != hipSuccess) return nullptr;
    s->tile_io = s->dev;
    s->pts = s->tile_io + tiles;
    s->evals = s->pts + OPEN_MAX_SEQ;
    s->scal = s->evals + OPEN_MAX_EVALS;
    s->h_up.resize((size_t)OPEN_MAX_BATCH * (2 + OPEN_TERMS));
    s->h_evals.resize(OPEN_MAX_EVALS);
    tls_open_scratch = std::move(s);
    return tls_open_scratch.get();
}

static bool open_shape_ok(uint64_t len, uint64_t group, uint64_t batch, int mode) {
    return len >= (mode == 1 ? 2u : 1u) && len <= OPEN_MAX_LEN && group >= 1 && batch >= 1 &&
           group <= OPEN_MAX_SEQ && batch <= OPEN_MAX_SEQ && group * batch <= OPEN_MAX_SEQ &&
           (mode == 0 || mode == 1);
}

// One batched Horner call on RNG_STREAM, all pointers on the device.  mode 0
// (reduce): evals[b*group + g] = the evaluation.  mode 1 (scan): q.out gets
// the len - 1 quotient coefficients of every sequence.  q.tiles is set here.
static int horner_dev(OpenScratch* os, OpenSeqs q, uint32_t batch, int mode, Fr* evals) {
    if (!open_shape_ok(q.len, q.group, batch, mode)) return RNG_ERR_BAD_ARG;
    const uint32_t nseq = batch * q.group;
    q.tiles = (q.len + OPEN_TILE - 1) / OPEN_TILE;
    if (q.tiles == 1) {
        if (mode == 0)
            hipLaunchKernelGGL((k_open_horner_tile<false, false>), dim3(nseq), dim3(OPEN_WG),
                               0, RNG_STREAM, q, evals);
        else
            hipLaunchKernelGGL((k_open_horner_tile<false, true>), dim3(nseq), dim3(OPEN_WG),
                               0, RNG_STREAM, q, (Fr*)nullptr);
        HIP_CHECK(hipGetLastError());
        return RNG_OK;
    }
    hipLaunchKernelGGL((k_open_horner_tile<false, false>), dim3(nseq * q.tiles),
                       dim3(OPEN_WG), 0, RNG_STREAM, q, os->tile_io);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_open_tile_prefix, dim3(nseq), dim3(OPEN_WG), 0, RNG_STREAM, q.pts,
                       q.pt_stride, q.group, q.tiles, os->tile_io,
                       mode == 0 ? evals : (Fr*)nullptr);
    HIP_CHECK(hipGetLastError());
    if (mode == 1) {
        hipLaunchKernelGGL((k_open_horner_tile<true, true>), dim3(nseq * q.tiles),
                           dim3(OPEN_WG), 0, RNG_STREAM, q, os->tile_io);
        HIP_CHECK(hipGetLastError());
    }
    return RNG_OK;
}

// Where the 11 polynomials of each of k proofs are on the device: wires 0..4
// and z as six slots of stride n + 3 per proof, the chunks as five.
struct OpenSrc {
    const Fr* wz;
    uint64_t wz_item;
    const Fr* chunks;
    uint64_t ch_item;
};

// Steps 1-3: the ten evaluations of every proof.  points = k x (zeta,
// zeta*w) on the host; on return (stream synchronized) os->h_evals holds
// 5k wire evaluations, then 4k sigma, then k of z.
static int open_evals_dev(const PlonkPkImpl& pk, const OpenSrc& src, uint32_t k,
                          const Fr* points, OpenScratch* os) {
    const uint32_t n = (uint32_t)pk.n;
    memcpy(os->h_up.data(), points, 2 * (size_t)k * sizeof(Fr));
    HIP_CHECK(hipMemcpyAsync(os->pts, os->h_up.data(), 2 * (size_t)k * sizeof(Fr),
                             hipMemcpyHostToDevice, RNG_STREAM));
    OpenSeqs q{};
    q.pts = os->pts;
    q.pt_stride = 2;
    q.src = src.wz, q.item_stride = src.wz_item, q.poly_stride = (uint64_t)n + 3;
    q.len = n + 2, q.group = 5;
    int rc = horner_dev(os, q, k, 0, os->evals);
    if (rc != RNG_OK) return rc;
    q.src = pk.coef_dev + 13 * (size_t)n, q.item_stride = 0, q.poly_stride = n;
    q.len = n, q.group = 4;
    rc = horner_dev(os, q, k, 0, os->evals + 5 * (size_t)k);
    if (rc != RNG_OK) return rc;
    q.pts = os->pts + 1;
    q.src = src.wz + 5 * ((size_t)n + 3), q.item_stride = src.wz_item;
    q.len = n + 3, q.group = 1;
    rc = horner_dev(os, q, k, 0, os->evals + 9 * (size_t)k);
    if (rc != RNG_OK) return rc;
    HIP_CHECK(hipMemcpyAsync(os->h_evals.data(), os->evals, 10 * (size_t)k * sizeof(Fr),
                             hipMemcpyDeviceToHost, RNG_STREAM));
    HIP_CHECK(hipStreamSynchronize(RNG_STREAM));
    return RNG_OK;
}

// Steps 5-7: C_p from the 29 scalars of each proof (into C, k x (n + 3)),
// then W_zeta = C_p / (X - zeta_p) and W_zeta_w = z_p / (X - zeta_p w) as two
// consecutive (n + 2)-coefficient blocks per proof in W.  points and scalars
// on the host; C and W on the device, neither aliasing a source.
static int open_combine_dev(const PlonkPkImpl& pk, const OpenSrc& src, uint32_t k,
                            const Fr* points, const Fr* scalars, Fr* C, Fr* W) {
    if (k < 1 || k > OPEN_MAX_BATCH || pk.n > OPEN_MAX_N) return RNG_ERR_BAD_ARG;
    OpenScratch* os = open_scratch_get();
    if (!os) return RNG_ERR_HIP;
    const uint32_t n = (uint32_t)pk.n;
    const size_t npts = 2 * (size_t)k, nsc = (size_t)OPEN_TERMS * k;
    memcpy(os->h_up.data(), points, npts * sizeof(Fr));
    memcpy(os->h_up.data() + npts, scalars, nsc * sizeof(Fr));
    HIP_CHECK(hipMemcpyAsync(os->pts, os->h_up.data(), npts * sizeof(Fr),
                             hipMemcpyHostToDevice, RNG_STREAM));
    HIP_CHECK(hipMemcpyAsync(os->scal, os->h_up.data() + npts, nsc * sizeof(Fr),
                             hipMemcpyHostToDevice, RNG_STREAM));
    OpenPolys P{pk.coef_dev, src.wz, src.wz_item, src.chunks, src.ch_item};
    hipLaunchKernelGGL(k_open_lincomb, dim3((n + 3 + 255) / 256, k), dim3(256), 0, RNG_STREAM,
                       P, (const Fr*)os->scal, C, n);
    HIP_CHECK(hipGetLastError());
    OpenSeqs q{};
    q.pts = os->pts;
    q.pt_stride = 2;
    q.src = C, q.item_stride = (uint64_t)n + 3;
    q.len = n + 3, q.group = 1;
    q.out = W, q.out_item_stride = 2 * ((uint64_t)n + 2);
    int rc = horner_dev(os, q, k, 1, nullptr);
    if (rc != RNG_OK) return rc;
    q.pts = os->pts + 1;
    q.src = src.wz + 5 * ((size_t)n + 3), q.item_stride = src.wz_item;
    q.out = W + ((size_t)n + 2);
    return horner_dev(os, q, k, 1, nullptr);
}

// The device stage of R4 + R5 for k proofs (st[0..k), zeta drawn): fills the
// evaluations and v of every state and leaves W_zeta, W_zeta_w of proof p in
// W blocks 2p, 2p + 1 for the caller's commit.  One stream sync, after the
// evaluations: the transcript and the linearization scalars are host work
// (on the pool for a cohort).
static int open_dev(const PlonkPkImpl& pk, const Fr& w, const OpenSrc& src, uint32_t k,
                    ProofState* st, Fr* C, Fr* W) {
    if (k < 1 || k > OPEN_MAX_BATCH || pk.n > OPEN_MAX_N) return RNG_ERR_BAD_ARG;
    OpenScratch* os = open_scratch_get();
    if (!os) return RNG_ERR_HIP;
    if (prover_env().cohort_trace || msm_env().debug) {
        fprintf(stderr, "[open_dev] n=%llu k=%u device stage\n", (unsigned long long)pk.n, k);
        fflush(stderr);
    }
    std::vector<Fr> points(2 * (size_t)k), scalars((size_t)OPEN_TERMS * k);
    for (uint32_t p = 0; p < k; ++p) {
        points[2 * (size_t)p] = st[p].zeta;
        points[2 * (size_t)p + 1] = st[p].zeta.mul(w);
    }
    int rc = open_evals_dev(pk, src, k, points.data(), os);
    if (rc != RNG_OK) return rc;
    const Fr* ev = os->h_evals.data();
    auto one = [&](uint32_t p) {
        ProofState& s = st[p];
        for (int j = 0; j < 5; ++j) s.wire_evals[j] = ev[5 * (size_t)p + j];
        for (int j = 0; j < 4; ++j) s.sigma_evals[j] = ev[5 * (size_t)k + 4 * (size_t)p + j];
        s.z_shift_eval = ev[9 * (size_t)k + p];
        absorb_evals(s);
        const LinScalars ls = lin_scalars(pk.k, pk.n, s.wire_evals, s.sigma_evals,
                                          s.z_shift_eval, s.beta, s.gamma, s.alpha, s.zeta);
        open_scalars(ls, s.v, scalars.data() + (size_t)OPEN_TERMS * p);
    };
    if (k > 1)
        HostPool::inst().parallel_for(k, one);
    else
        one(0);
    return open_combine_dev(pk, src, k, points.data(), scalars.data(), C, W);
}

// ---------------- the prover: cohorts of k >= 1 proofs ----------------
// The reference proves many jobs concurrently from a rayon pool
// (native_proof_manager.rs:143-148,193-198).  Per-proof GPU runs at n=4096
// are aggregation-latency chains (r01 profile: window_combine 30% +
// seg_merge 22% of proof-workload GPU time), so the prover advances k
// proofs in LOCKSTEP — R1 for all, R2 for all, … — and fuses each round's
// commitments into ONE msm_dev_run (key group g = poly*W + window already
// supports a batch dimension).  Transcripts and blinders stay per-proof (one
// ProofState each, which consumes only its own commitments, through the
// host rounds of plonk_rounds.hpp), so a proof's bytes depend on its seed
// and inputs alone, not on k or its place in the cohort; rng_prove is the
// cohort of one.  Host-side phases (grand product, evaluations,
// linearization) run on a persistent worker pool (HostPool, defined before
// msm_dev_run so its window fold can use it).

struct CohortScratch {  // per-thread device scratch of the prover
    uint64_t elems = 0, k = 0;  // capacity: k*(n+3) of the largest call, and k
    Fr* stage = nullptr;     // max(5k*(n+3), k*m) staging for commits/NTTs
    uint64_t stage_elems = 0;
    uint64_t* canon = nullptr;  // canonical scalars for the fused MSM
    Fr* coset_in = nullptr;  // 7k*(n+3) coefficient staging for the coset batch
    Fr* coset_out = nullptr; // 7k*m coset evaluations (5 wires + z + PI per proof)
    Fr* q_all = nullptr;     // k*m quotient evals
    Fr* ntt_tmp = nullptr;   // 7k*m NTT ping-pong
    QuotChal* chs = nullptr;  // k challenge packs (batched quotient)
    Fr* blinders = nullptr;   // 10k wire + 4k chunk blinders (device)
    ~CohortScratch() {
        for (void* b : {(void*)stage, (void*)canon, (void*)coset_in, (void*)coset_out,
                        (void*)q_all, (void*)ntt_tmp, (void*)chs, (void*)blinders})
            hip_free_guarded(b);
    }
};

static thread_local std::unique_ptr<CohortScratch> tls_cohort_scratch;

static int cohort_scratch_ensure(uint64_t n, uint64_t k) {
    // Every buffer is linear in e = k*(n+3) (k*m = 8kn < 8e), bar the two
    // that are linear in k.  Grow each capacity to the max of old and new: a
    // mixed-circuit stream (service batcher: n=4096 settlements between
    // n=16384 validities) would otherwise thrash reallocations between
    // shapes, and the scratch stays bounded by the largest single call (one
    // n=2^17 proof, then 128 at n=4096, is not 128 x 2^17).
    uint64_t e = k * (n + 3);
    if (tls_cohort_scratch && tls_cohort_scratch->elems >= e && tls_cohort_scratch->k >= k)
        return RNG_OK;
    if (tls_cohort_scratch) {
        if (tls_cohort_scratch->elems > e) e = tls_cohort_scratch->elems;
        if (tls_cohort_scratch->k > k) k = tls_cohort_scratch->k;
    }
    const uint64_t km = 8 * e;
    tls_cohort_scratch = std::make_unique<CohortScratch>();
    CohortScratch* s = tls_cohort_scratch.get();
    uint64_t stage_elems = 5 * e;
    if (stage_elems < km) stage_elems = km;
    HIP_CHECK(hipMalloc(&s->stage, stage_elems * sizeof(Fr)));
    HIP_CHECK(hipMalloc(&s->canon, stage_elems * 4 * 8));
    HIP_CHECK(hipMalloc(&s->coset_in, 7 * e * sizeof(Fr)));
    HIP_CHECK(hipMalloc(&s->coset_out, 7 * km * sizeof(Fr)));
    HIP_CHECK(hipMalloc(&s->q_all, km * sizeof(Fr)));
    HIP_CHECK(hipMalloc(&s->ntt_tmp, 7 * km * sizeof(Fr)));
    HIP_CHECK(hipMalloc(&s->chs, k * sizeof(QuotChal)));
    HIP_CHECK(hipMalloc(&s->blinders, 14 * k * sizeof(Fr)));
    s->stage_elems = stage_elems;
    s->elems = e;
    s->k = k;
    return RNG_OK;
}

// round-1 commit on the Lagrange path: d_canon already holds B blocks of
// n + 2 canonical scalars (k_lagrange_scalars).  MSM_LAGRANGE_UNUSABLE tells
// the caller to commit the staged coefficients instead.
static int commit_lagrange_canon(RngCtxImpl* ctx, uint64_t n, const uint64_t* d_canon,
                                 uint32_t B, G1Aff* out, bool* out_inf) {
    std::vector<G1Jac> res(B);
    int rc = msm_lagrange_run(ctx, n, d_canon, B, res.data());
    if (rc != RNG_OK) return rc;
    jacs_to_affine(res.data(), B, out, out_inf);
    return RNG_OK;
}

// the quotient kernels' challenge pack: the part fixed by the key (coset
// shifts, 1/Z_H on the 8 cosets of the 8n domain), then one proof's challenges
static QuotChal quot_chal_fixed(const PlonkPkImpl& pk) {
    QuotChal ch{};
    for (int j = 0; j < 5; ++j) ch.k[j] = pk.k[j];
    Fr g = Fr::from_u64(FR_GENERATOR);
    Fr gn = g.pow_u64(pk.n);
    Fr w8 = h_fr_root_of_unity((uint32_t)(8 * pk.n)).pow_u64(pk.n);
    std::vector<Fr> zh(8);
    Fr cur = gn;
    for (int t = 0; t < 8; ++t) {
        zh[t] = cur.sub(Fr::one());
        cur = cur.mul(w8);
    }
    zh = hbatch_inverse(zh);
    for (int t = 0; t < 8; ++t) ch.zh_inv[t] = zh[t];
    return ch;
}
static void quot_chal_set(QuotChal& ch, const ProofState& st) {
    ch.beta = st.beta;
    ch.gamma = st.gamma;
    ch.alpha = st.alpha;
    ch.alpha2 = st.alpha.sqr();
}

// Round 3 up to the chunk commit, for k proofs: cs->coset_in holds k x 7
// coefficient polynomials at stride n+3 (wires 0..4, z, PI) on entry; on
// return cs->stage holds the 5k blinded chunks at stride n+3 and cs->ntt_tmp
// the k x m quotient coefficients.  out_of_place keeps coset_in plain (the
// device R4 + R5 read it again); otherwise it is scaled in place.  chs_h: k
// challenge packs, qblind_h: 4k chunk blinders, both host; the caller keeps
// qblind_h alive until its next synchronisation of RNG_STREAM.  The prover
// and rng_quotient_pk both come through here.
static int quotient_stage(RngCtxImpl* ctx, const PlonkPkImpl& pk, uint32_t k,
                          CohortScratch* cs, bool out_of_place, const QuotChal* chs_h,
                          const Fr* qblind_h) {
    const uint64_t n = pk.n;
    const uint32_t m = (uint32_t)(8 * n);
    NttPlan* mp = get_plan(ctx, m, 0);  // tables only; batch NTTs below
    if (!mp || ensure_coset_tables(ctx, mp) != RNG_OK) return RNG_ERR_HIP;
    const uint64_t stride = n + 3;
    uint64_t total_in = 7 * (uint64_t)k * stride;
    uint64_t total_m = 7 * (uint64_t)k * m;
    if (out_of_place) {
        // R4 + R5 read the plain coefficients again: scale while padding,
        // out of place
        hipLaunchKernelGGL(k_scale_pad_batch, dim3((uint32_t)((total_m + 255) / 256)),
                           dim3(256), 0, RNG_STREAM, (const Fr*)cs->coset_in,
                           (uint32_t)stride, (const Fr*)mp->gpow, cs->ntt_tmp, m,
                           total_m);
        HIP_CHECK(hipGetLastError());
    } else {
        hipLaunchKernelGGL(k_mul_pointwise_mod,
                           dim3((uint32_t)((total_in + 255) / 256)), dim3(256), 0,
                           RNG_STREAM, cs->coset_in, mp->gpow, (uint32_t)stride,
                           total_in);
        HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_copy_pad_batch, dim3((uint32_t)((total_m + 255) / 256)),
                           dim3(256), 0, RNG_STREAM, cs->coset_in, (uint32_t)stride,
                           cs->ntt_tmp, m, total_m);
        HIP_CHECK(hipGetLastError());
    }
    int rc = ntt_dev_run(ctx, cs->ntt_tmp, cs->coset_out, m, 7 * (uint64_t)k, false,
                         RNG_STREAM);
    if (rc != RNG_OK) return rc;

    // ONE batched quotient launch for all k proofs (a single proof's m
    // grid is latency-starved; 483 small launches were 14% of cohort GPU
    // time in the r02 profile)
    {
        HIP_CHECK(hipMemcpyAsync(cs->chs, chs_h, k * sizeof(QuotChal),
                                 hipMemcpyHostToDevice, RNG_STREAM));
        uint64_t total_kq = (uint64_t)k * m;
        hipLaunchKernelGGL(k_quotient_batch,
                           dim3((uint32_t)((total_kq + 255) / 256)), dim3(256), 0,
                           RNG_STREAM, pk.sel_coset, pk.sig_coset, cs->coset_out,
                           pk.l1_coset, mp->xpow, cs->q_all, m, k, cs->chs);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(RNG_STREAM));  // chs_h lifetime
    }
    // batched inverse coset NTT of the k quotients
    rc = ntt_dev_run(ctx, cs->q_all, cs->ntt_tmp, m, k, true, RNG_STREAM);
    if (rc != RNG_OK) return rc;
    uint64_t total_q = (uint64_t)k * m;
    hipLaunchKernelGGL(k_mul_pointwise_mod, dim3((uint32_t)((total_q + 255) / 256)),
                       dim3(256), 0, RNG_STREAM, cs->ntt_tmp, mp->gpow_inv, m,
                       total_q);
    HIP_CHECK(hipGetLastError());
    // chunk-split + linking blinders ON DEVICE, into the commit's staging
    HIP_CHECK(hipMemcpyAsync(cs->blinders, qblind_h, 4 * (size_t)k * sizeof(Fr),
                             hipMemcpyHostToDevice, RNG_STREAM));
    uint64_t total_c = 5 * (uint64_t)k * (n + 3);
    hipLaunchKernelGGL(k_quot_chunks_batch,
                       dim3((uint32_t)((total_c + 255) / 256)), dim3(256), 0,
                       RNG_STREAM, cs->ntt_tmp, cs->blinders, cs->stage,
                       (uint32_t)n, m, total_c);
    HIP_CHECK(hipGetLastError());
    return RNG_OK;
}

// k >= 1 proofs in lockstep under ONE proving key (the headline shape: a
// stream of same-circuit jobs); the only prover, behind rng_prove (k = 1) and
// rng_prove_cohort.  One ProofState per proof runs the shared host rounds of
// plonk_rounds.hpp, so a proof's bytes do not depend on k.  4 fused MSM runs
// per cohort instead of 5k.
static int plonk_prove_impl(RngCtxImpl* ctx, const PlonkPkImpl& pk, uint32_t k,
                            const Fr* wires_all, const Fr* pubs_all, const uint64_t* seeds,
                            uint64_t* out_proofs, uint64_t* out_hints) {
    const uint64_t n = pk.n;
    const uint32_t m = (uint32_t)(8 * n);
    const uint64_t hint_u64s = 4 * (n + 2) + 9;
    const int trace = prover_env().cohort_trace;
    auto t_enter = std::chrono::steady_clock::now();
#define COHORT_TRACE(tag)                                                     \
    do {                                                                      \
        if (trace) {                                                          \
            double ms_ = std::chrono::duration<double, std::milli>(           \
                             std::chrono::steady_clock::now() - t_enter)      \
                             .count();                                        \
            fprintf(stderr, "[cohort +%7.2fms] %s\n", ms_, tag);              \
            fflush(stderr);                                                   \
        }                                                                     \
    } while (0)
    COHORT_TRACE("enter");
    if (!cosets_ok(n)) return RNG_ERR_BAD_ARG;
    if (cohort_scratch_ensure(n, k) != RNG_OK) return RNG_ERR_HIP;
    CohortScratch* cs = tls_cohort_scratch.get();
    HostPool& pool = HostPool::inst();
    Fr w = h_fr_root_of_unity((uint32_t)n);
    const bool z_dev =
        ProverEnv::on(prover_env().z_device, Z_DEVICE_DEFAULT) && n <= PERM_MAX_N;
    // R4 + R5 on the device: the blinded polynomials stay on the device (the
    // wires and z as plain coefficients in coset_in, the chunks in stage) and
    // only wire 0 comes down, for a link hint
    const bool open_on =
        ProverEnv::on(prover_env().open_device, OPEN_DEVICE_DEFAULT) && n <= OPEN_MAX_N;

    std::vector<ProofState> st;
    st.reserve(k);
    for (uint32_t p = 0; p < k; ++p)
        st.emplace_back(pk, pubs_all + (size_t)p * pk.npub, seeds[p]);
    // one round's blinders of every proof, packed for the upload
    auto pack_blinders = [&](int first, int count) {
        std::vector<Fr> h((size_t)count * k);
        for (uint32_t p = 0; p < k; ++p)
            for (int i = 0; i < count; ++i) h[(size_t)count * p + i] = st[p].blind[first + i];
        return h;
    };

    // one round's commitments, before the states take them
    std::vector<G1Aff> cbuf(5 * (size_t)k);
    std::unique_ptr<bool[]> ibuf(new bool[5 * (size_t)k]);
    std::vector<const std::vector<Fr>*> ps(5 * (size_t)k);

    COHORT_TRACE("r1");
    // --- R1: wire polys (one batched IFFT + one fused MSM) ---
    {
        if (z_dev) {
            // the IFFT and the blinding below overwrite stage, and R2's device
            // grand product needs the evaluations again: upload into
            // coset_out (unused until R3, so no extra memory) and stage a copy
            HIP_CHECK(hipMemcpyAsync(cs->coset_out, wires_all,
                                     (size_t)5 * k * n * sizeof(Fr),
                                     hipMemcpyHostToDevice, RNG_STREAM));
            HIP_CHECK(hipMemcpyAsync(cs->stage, cs->coset_out,
                                     (size_t)5 * k * n * sizeof(Fr),
                                     hipMemcpyDeviceToDevice, RNG_STREAM));
        } else {
            HIP_CHECK(hipMemcpyAsync(cs->stage, wires_all, (size_t)5 * k * n * sizeof(Fr),
                                     hipMemcpyHostToDevice, RNG_STREAM));
        }
        std::vector<Fr> blind_h = pack_blinders(BLIND_WIRES, 10);
        HIP_CHECK(hipMemcpyAsync(cs->blinders, blind_h.data(),
                                 blind_h.size() * sizeof(Fr), hipMemcpyHostToDevice,
                                 RNG_STREAM));
        const bool lagrange =
            ProverEnv::on(prover_env().r1_lagrange, k >= R1_LAGRANGE_MIN_K);
        if (lagrange) {
            // the commitment MSM reads the (sparse) evaluations and the
            // blinders as scalars against the Lagrange bases: canonicalise
            // them before the IFFT overwrites stage
            uint64_t lt = 5 * (uint64_t)k * (n + 2);
            hipLaunchKernelGGL(k_lagrange_scalars, dim3((uint32_t)((lt + 255) / 256)),
                               dim3(256), 0, RNG_STREAM, (const Fr*)cs->stage,
                               (const Fr*)cs->blinders, (uint32_t)n, lt, cs->canon);
            HIP_CHECK(hipGetLastError());
        }
        COHORT_TRACE("r1-ifft");
        int rc = ntt_dev_run(ctx, cs->stage, cs->ntt_tmp, (uint32_t)n, 5 * (uint64_t)k,
                             true, RNG_STREAM);
        if (rc != RNG_OK) return rc;
        COHORT_TRACE("r1-ifft-done");
        // blind + pad ON DEVICE, commit straight from the staged device
        // buffers; the blinded coefficients stream back D2H on the same
        // stream and are complete once the commit's internal sync returns
        uint64_t total1 = 5 * (uint64_t)k * (n + 3);
        hipLaunchKernelGGL(k_blind_wires_batch,
                           dim3((uint32_t)((total1 + 255) / 256)), dim3(256), 0,
                           RNG_STREAM, cs->ntt_tmp, cs->blinders, cs->stage,
                           cs->coset_in, (uint32_t)n, total1);
        HIP_CHECK(hipGetLastError());
        uint64_t wlen = 5 * (uint64_t)k * (n + 2);
        std::vector<Fr> host_flat(open_on ? (out_hints ? (size_t)k * (n + 2) : 0) : wlen);
        if (!open_on)
            HIP_CHECK(hipMemcpyAsync(host_flat.data(), cs->stage, wlen * sizeof(Fr),
                                     hipMemcpyDeviceToHost, RNG_STREAM));
        else if (out_hints)  // wire 0 of every proof: one row in five
            HIP_CHECK(hipMemcpy2DAsync(host_flat.data(), (n + 2) * sizeof(Fr), cs->stage,
                                       5 * (n + 2) * sizeof(Fr), (n + 2) * sizeof(Fr), k,
                                       hipMemcpyDeviceToHost, RNG_STREAM));
        COHORT_TRACE("r1-sync-done");
        int crc = lagrange ? commit_lagrange_canon(ctx, n, cs->canon, 5 * k, cbuf.data(),
                                                   ibuf.get())
                           : MSM_LAGRANGE_UNUSABLE;
        if (crc == MSM_LAGRANGE_UNUSABLE)  // coefficient path
            crc = commit_staged(ctx, cs->stage, cs->canon, n + 2, 5 * k, cbuf.data(), ibuf.get());
        if (crc != RNG_OK) return RNG_ERR_HIP;
        pool.parallel_for(k, [&](uint32_t p) {
            if (open_on) {
                if (out_hints) {
                    const Fr* src = host_flat.data() + (size_t)p * (n + 2);
                    st[p].wpoly[0].assign(src, src + (n + 2));
                }
                return;
            }
            for (int j = 0; j < 5; ++j) {
                const Fr* src = host_flat.data() + ((size_t)5 * p + j) * (n + 2);
                st[p].wpoly[j].assign(src, src + (n + 2));
            }
        });
        COHORT_TRACE("r1-blind-done");
        pool.parallel_for(k, [&](uint32_t p) {
            st[p].take_comms(COMM_WIRES, 5, &cbuf[5 * (size_t)p], &ibuf[5 * (size_t)p]);
            if (out_hints) st[p].write_link_hint(out_hints + (size_t)p * hint_u64s);
            st[p].beta = st[p].tr.challenge();
            st[p].gamma = st[p].tr.challenge();
        });
    }

    COHORT_TRACE("r2");
    // --- R2: grand products (device stage or host pool) + batched IFFT of
    //     z and PI ---
    {
        // stage = k z-cols then k PI-cols; the device stage writes the z half
        // in place (terms and scans in q_all, free until R3), so only the
        // PI half is uploaded
        std::vector<Fr> evals_flat((z_dev ? 1 : 2) * (size_t)k * n);
        Fr* pi_base = evals_flat.data() + (z_dev ? 0 : (size_t)k * n);
        pool.parallel_for(k, [&](uint32_t p) {
            if (!z_dev)
                perm_product_host(pk, w, wires_all + (size_t)5 * p * n, st[p].beta,
                                  st[p].gamma, evals_flat.data() + (size_t)p * n);
            Fr* pie = pi_base + (size_t)p * n;
            for (uint64_t i = 0; i < n; ++i) pie[i] = Fr::zero();
            const Fr* pubs = pubs_all + (size_t)p * pk.npub;
            for (uint64_t i = 0; i < pk.npub; ++i) pie[i] = pubs[i];
        });
        if (z_dev) {
            std::vector<Fr> bg(2 * (size_t)k);
            for (uint32_t p = 0; p < k; ++p) {
                bg[2 * (size_t)p] = st[p].beta;
                bg[2 * (size_t)p + 1] = st[p].gamma;
            }
            int prc = perm_product_dev(cs->coset_out, pk.sig_evals_dev, pk.wpow_dev, pk.k,
                                       bg.data(), n, k, cs->q_all, cs->stage);
            if (prc != RNG_OK) return prc;
            HIP_CHECK(hipMemcpyAsync(cs->stage + (size_t)k * n, evals_flat.data(),
                                     (size_t)k * n * sizeof(Fr), hipMemcpyHostToDevice,
                                     RNG_STREAM));
        } else {
            HIP_CHECK(hipMemcpyAsync(cs->stage, evals_flat.data(),
                                     2 * (size_t)k * n * sizeof(Fr),
                                     hipMemcpyHostToDevice, RNG_STREAM));
        }
        int rc = ntt_dev_run(ctx, cs->stage, cs->ntt_tmp, (uint32_t)n, 2 * (uint64_t)k,
                             true, RNG_STREAM);
        if (rc != RNG_OK) return rc;
        // device-side z blinding + PI staging straight into the R3 coset
        // slots (the wires landed there in R1)
        std::vector<Fr> zblind_h = pack_blinders(BLIND_Z, 3);
        HIP_CHECK(hipMemcpyAsync(cs->blinders, zblind_h.data(),
                                 zblind_h.size() * sizeof(Fr),
                                 hipMemcpyHostToDevice, RNG_STREAM));
        uint64_t totz = (uint64_t)k * (n + 3);
        hipLaunchKernelGGL(k_blind_z_batch, dim3((uint32_t)((totz + 255) / 256)),
                           dim3(256), 0, RNG_STREAM, cs->ntt_tmp, cs->blinders,
                           cs->stage, cs->coset_in, (uint32_t)n, totz);
        HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_pi_to_coset, dim3((uint32_t)((totz + 255) / 256)),
                           dim3(256), 0, RNG_STREAM,
                           cs->ntt_tmp + (size_t)k * n, cs->coset_in, (uint32_t)n,
                           totz);
        HIP_CHECK(hipGetLastError());
        std::vector<Fr> z_host(open_on ? 0 : totz);
        if (!open_on)
            HIP_CHECK(hipMemcpyAsync(z_host.data(), cs->stage, totz * sizeof(Fr),
                                     hipMemcpyDeviceToHost, RNG_STREAM));
        if (commit_staged(ctx, cs->stage, cs->canon, n + 3, k, cbuf.data(), ibuf.get()) != RNG_OK)
            return RNG_ERR_HIP;
        // commit_staged synchronized: z_host is complete
        pool.parallel_for(k, [&](uint32_t p) {
            if (!open_on) {
                const Fr* src = z_host.data() + (size_t)p * (n + 3);
                st[p].zpoly.assign(src, src + (n + 3));
            }
            st[p].take_comms(COMM_Z, 1, &cbuf[p], &ibuf[p]);
            st[p].alpha = st[p].tr.challenge();
        });
    }

    COHORT_TRACE("r3");
    // --- R3: coset transforms (batched) + quotient + fused MSM ---
    {
        std::vector<QuotChal> chs_h(k, quot_chal_fixed(pk));
        for (uint32_t p = 0; p < k; ++p) quot_chal_set(chs_h[p], st[p]);
        std::vector<Fr> qblind_h = pack_blinders(BLIND_CHUNKS, 4);
        int rc = quotient_stage(ctx, pk, k, cs, open_on, chs_h.data(), qblind_h.data());
        if (rc != RNG_OK) return rc;
        // the blinded chunks stream back D2H for the host R5 linearization
        // (complete after the commit's internal sync)
        uint64_t total_c = 5 * (uint64_t)k * (n + 3);
        std::vector<Fr> chunks_host(open_on ? 0 : total_c);
        if (!open_on)
            HIP_CHECK(hipMemcpyAsync(chunks_host.data(), cs->stage,
                                     total_c * sizeof(Fr), hipMemcpyDeviceToHost,
                                     RNG_STREAM));
        if (commit_staged(ctx, cs->stage, cs->canon, n + 3, 5 * k, cbuf.data(), ibuf.get()) != RNG_OK)
            return RNG_ERR_HIP;
        if (!open_on)
            pool.parallel_for(k, [&](uint32_t p) {
                for (int i = 0; i < 5; ++i) {
                    const Fr* src = chunks_host.data() + (5 * (size_t)p + i) * (n + 3);
                    st[p].quot_chunks[i].assign(src, src + (i < 4 ? n + 3 : n + 2));
                }
            });
        pool.parallel_for(k, [&](uint32_t p) {
            st[p].take_comms(COMM_CHUNKS, 5, &cbuf[5 * (size_t)p], &ibuf[5 * (size_t)p]);
            st[p].zeta = st[p].tr.challenge();
        });
    }

    COHORT_TRACE("r4r5");
    // --- R4 + R5: evaluations, linearization, openings (device stage or
    //     host pool) ---
    if (open_on) {
        // coset_out, q_all and ntt_tmp are free after the chunk split: C goes
        // to q_all, W_zeta / W_zeta_w to ntt_tmp, and the commit reads them
        // there (no host packing, no upload)
        const OpenSrc src{cs->coset_in, 7 * (n + 3), cs->stage, 5 * (n + 3)};
        int orc = open_dev(pk, w, src, k, st.data(), cs->q_all, cs->ntt_tmp);
        if (orc != RNG_OK) return orc;
        if (commit_staged(ctx, cs->ntt_tmp, cs->canon, n + 2, 2 * k, cbuf.data(),
                          ibuf.get()) != RNG_OK)
            return RNG_ERR_HIP;
    } else {
        std::vector<std::vector<Fr>> Wz(k), Wzw(k);
        pool.parallel_for(k, [&](uint32_t p) { rounds_4_5(pk, w, st[p], Wz[p], Wzw[p]); });
        for (uint32_t p = 0; p < k; ++p) {
            ps[2 * (size_t)p] = &Wz[p];
            ps[2 * (size_t)p + 1] = &Wzw[p];
        }
        if (commit_host_polys(ctx, ps.data(), 2 * k, cs->stage, cs->canon, cs->stage_elems,
                              cbuf.data(), ibuf.get()) != RNG_OK)
            return RNG_ERR_HIP;
    }
    pool.parallel_for(k, [&](uint32_t p) {
        st[p].take_comms(COMM_WZ, 2, &cbuf[2 * (size_t)p], &ibuf[2 * (size_t)p]);
        st[p].serialize(out_proofs + (size_t)p * 157);
    });
    return RNG_OK;
}

// upload host coeffs, pad to m, coset-forward into dst (device, m elems)
static int coset_of_coeffs(RngCtxImpl* ctx, const std::vector<Fr>& coeffs, Fr* dst,
                           uint32_t m) {
    ProveScratch* s = tls_prove_scratch.get();
    HIP_CHECK(hipMemcpyAsync(s->stage, coeffs.data(), coeffs.size() * sizeof(Fr),
                             hipMemcpyHostToDevice, RNG_STREAM));
    uint32_t blocks = (m + 255) / 256;
    hipLaunchKernelGGL(k_copy_pad, dim3(blocks), dim3(256), 0, RNG_STREAM, s->stage,
                       (uint32_t)coeffs.size(), s->tmp, m);
    HIP_CHECK(hipGetLastError());
    return coset_fwd_dev(ctx, s->tmp, dst, m);
}

// GPU batched IFFT of column-major evals (host) -> host coeff vectors
static int ifft_columns(RngCtxImpl* ctx, const Fr* host_evals, uint64_t n,
                        uint64_t ncols, std::vector<Fr>* out_cols) {
    Fr* d = nullptr;
    HIP_CHECK(hipMalloc(&d, 2 * n * ncols * sizeof(Fr)));
    if (hipMemcpyAsync(d, host_evals, n * ncols * sizeof(Fr), hipMemcpyHostToDevice,
                       RNG_STREAM) != hipSuccess) {
        hipFree(d);
        return RNG_ERR_HIP;
    }
    Fr* out = (n <= NTT_SMALL_MAX) ? d : d + n * ncols;
    int rc = ntt_dev_run(ctx, d, out, (uint32_t)n, ncols, true, RNG_STREAM);
    if (rc == RNG_OK) {
        for (uint64_t c = 0; c < ncols; ++c) {
            out_cols[c].resize(n);
            if (hipMemcpyAsync(out_cols[c].data(), out + c * n, n * sizeof(Fr),
                               hipMemcpyDeviceToHost, RNG_STREAM) != hipSuccess)
                rc = RNG_ERR_HIP;
        }
        if (hipStreamSynchronize(RNG_STREAM) != hipSuccess) rc = RNG_ERR_HIP;
    }
    hipFree(d);
    return rc;
}

static int plonk_preprocess_impl(RngCtxImpl* ctx, const RngCircuitDesc* d,
                                 PlonkPkImpl* pk) {
    const uint64_t n = d->n, m = 8 * n;
    pk->n = n;
    pk->npub = d->num_public;
    coset_ks(pk->k);
    if (!cosets_ok(n)) return RNG_ERR_BAD_ARG;
    if (prove_scratch_ensure(n) != RNG_OK) return RNG_ERR_HIP;

    // selector + sigma polynomials (GPU IFFT)
    if (ifft_columns(ctx, (const Fr*)d->selectors, n, 13, pk->selq) != RNG_OK)
        return RNG_ERR_HIP;
    // sigma evals from permutation indices
    Fr w = h_fr_root_of_unity((uint32_t)n);
    std::vector<Fr> wpow(n);
    wpow[0] = Fr::one();
    for (uint64_t i = 1; i < n; ++i) wpow[i] = wpow[i - 1].mul(w);
    std::vector<Fr> sig_evals_flat(5 * n);
    for (int j = 0; j < 5; ++j) {
        for (uint64_t i = 0; i < n; ++i) {
            uint64_t slot = d->sigma[(size_t)j * n + i];
            sig_evals_flat[(size_t)j * n + i] = pk->k[slot / n].mul(wpow[slot % n]);
        }
        pk->sig_evals[j].assign(sig_evals_flat.begin() + (size_t)j * n,
                                sig_evals_flat.begin() + (size_t)(j + 1) * n);
    }
    if (ifft_columns(ctx, sig_evals_flat.data(), n, 5, pk->sigp) != RNG_OK)
        return RNG_ERR_HIP;
    // device tables of the grand-product stage (6n Fr per key)
    HIP_CHECK(hipMalloc(&pk->sig_evals_dev, 5 * n * sizeof(Fr)));
    HIP_CHECK(hipMalloc(&pk->wpow_dev, n * sizeof(Fr)));
    HIP_CHECK(hipMemcpy(pk->sig_evals_dev, sig_evals_flat.data(), 5 * n * sizeof(Fr),
                        hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(pk->wpow_dev, wpow.data(), n * sizeof(Fr), hipMemcpyHostToDevice));
    // coefficient forms for the R4 + R5 stage (18n Fr per key)
    HIP_CHECK(hipMalloc(&pk->coef_dev, 18 * n * sizeof(Fr)));
    for (int s = 0; s < 18; ++s)
        HIP_CHECK(hipMemcpy(pk->coef_dev + (size_t)s * n,
                            s < 13 ? pk->selq[s].data() : pk->sigp[s - 13].data(),
                            n * sizeof(Fr), hipMemcpyHostToDevice));

    // commitments (two fused batch MSMs)
    {
        const std::vector<Fr>* ps[13];
        for (int s = 0; s < 13; ++s) ps[s] = &pk->selq[s];
        if (commit_dev_batch(ctx, ps, 13, pk->sel_comms, pk->sel_inf) != RNG_OK)
            return RNG_ERR_HIP;
        for (int j = 0; j < 5; ++j) ps[j] = &pk->sigp[j];
        if (commit_dev_batch(ctx, ps, 5, pk->sig_comms, pk->sig_inf) != RNG_OK)
            return RNG_ERR_HIP;
    }

    // coset caches
    HIP_CHECK(hipMalloc(&pk->sel_coset, 13 * m * sizeof(Fr)));
    HIP_CHECK(hipMalloc(&pk->sig_coset, 5 * m * sizeof(Fr)));
    HIP_CHECK(hipMalloc(&pk->l1_coset, m * sizeof(Fr)));
    for (int s = 0; s < 13; ++s)
        if (coset_of_coeffs(ctx, pk->selq[s], pk->sel_coset + (size_t)s * m, (uint32_t)m) !=
            RNG_OK)
            return RNG_ERR_HIP;
    for (int j = 0; j < 5; ++j)
        if (coset_of_coeffs(ctx, pk->sigp[j], pk->sig_coset + (size_t)j * m, (uint32_t)m) !=
            RNG_OK)
            return RNG_ERR_HIP;
    {
        // L1 = IFFT(e0)
        std::vector<Fr> e0(n, Fr::zero());
        e0[0] = Fr::one();
        std::vector<Fr> l1coef[1];
        if (ifft_columns(ctx, e0.data(), n, 1, l1coef) != RNG_OK) return RNG_ERR_HIP;
        if (coset_of_coeffs(ctx, l1coef[0], pk->l1_coset, (uint32_t)m) != RNG_OK)
            return RNG_ERR_HIP;
    }
    HIP_CHECK(hipDeviceSynchronize());
    return RNG_OK;
}

}  // namespace rng

// ---------------- C ABI ----------------

using namespace rng;

struct RngCtx {
    RngCtxImpl impl;
};

extern "C" {

const char* rng_version(void) { return "renegade_amd 0.1 (gfx950)"; }

int rng_gpu_available(void) { return gpu_ok() ? 1 : 0; }

/* Join the host worker pool's threads (harmless if never started).  Call
 * before process exit under a profiler: rocprofv3's finalizer can stall on
 * live foreign threads.  Subsequent pool work runs serially. */
void rng_shutdown_pool(void) { HostPool::inst().stop(); }

int rng_set_device(int device) {
    if (!gpu_ok()) return RNG_ERR_NO_GPU;
    hipError_t e = hipSetDevice(device);
    (void)hipGetLastError();  // clear the sticky last-error slot on failure
    return e == hipSuccess ? RNG_OK : RNG_ERR_HIP;
}

int rng_msm_last_times(double out_ms[5]) {
    for (int i = 0; i < 5; ++i) out_ms[i] = tls_msm_times[i];
    return 5;
}
int rng_ntt_last_times(double out_ms[2]) {
    for (int i = 0; i < 2; ++i) out_ms[i] = tls_ntt_times[i];
    return 2;
}

RngCtx* rng_prover_init(const uint8_t* srs_ptau, size_t len, uint64_t max_degree) {
    if (!srs_ptau || len < 12) return nullptr;
    auto ctx = std::make_unique<RngCtx>();
    RngCtxImpl* im = &ctx->impl;
    // --- parse ptau (semantics of srs.rs:63-214) ---
    size_t pos = 0;
    auto rd_u32 = [&](uint32_t* v) {
        if (pos + 4 > len) return false;
        memcpy(v, srs_ptau + pos, 4);
        pos += 4;
        return true;
    };
    auto rd_u64 = [&](uint64_t* v) {
        if (pos + 8 > len) return false;
        memcpy(v, srs_ptau + pos, 8);
        pos += 8;
        return true;
    };
    if (memcmp(srs_ptau, "ptau", 4) != 0) return nullptr;
    pos = 4;
    uint32_t version, nsections;
    if (!rd_u32(&version) || version != 1) return nullptr;
    if (!rd_u32(&nsections) || nsections != 11) return nullptr;
    uint32_t secnum;
    uint64_t secsize;
    if (!rd_u32(&secnum) || secnum != 1 || !rd_u64(&secsize)) return nullptr;
    size_t s1_end = pos + secsize;
    uint32_t n8;
    if (!rd_u32(&n8) || n8 != 32) return nullptr;
    static const u64 qmod[4] = FQ_MODULUS;
    if (pos + 32 > len || memcmp(srs_ptau + pos, qmod, 32) != 0) return nullptr;
    pos += 32;
    uint32_t power, cpower;
    if (!rd_u32(&power) || !rd_u32(&cpower)) return nullptr;
    if ((1ull << power) + 2 < max_degree) return nullptr;
    pos = s1_end;
    if (!rd_u32(&secnum) || secnum != 2 || !rd_u64(&secsize)) return nullptr;
    size_t s2_end = pos + secsize;
    uint64_t npoints = max_degree + 1;
    if (pos + npoints * 64 > len) return nullptr;
    im->srs_g1_host.resize(npoints * 8);
    memcpy(im->srs_g1_host.data(), srs_ptau + pos, npoints * 64);
    // curve-membership check (srs.rs:179) on a sample + endpoints; full check
    // deferred to the GPU parity tests to keep init latency low.
    {
        static const u64 bmont[4] = G1_B_MONT;
        Fq b;
        memcpy(b.l, bmont, 32);
        for (uint64_t i : {uint64_t(0), npoints / 2, npoints - 1}) {
            Fq x, y;
            memcpy(x.l, &im->srs_g1_host[i * 8], 32);
            memcpy(y.l, &im->srs_g1_host[i * 8 + 4], 32);
            if (!y.sqr().eq(x.sqr().mul(x).add(b))) return nullptr;
        }
    }
    pos = s2_end;
    if (!rd_u32(&secnum) || secnum != 3 || !rd_u64(&secsize)) return nullptr;
    if (pos + 2 * 128 > len) return nullptr;
    memcpy(im->h_g2, srs_ptau + pos, 128);
    memcpy(im->beta_h_g2, srs_ptau + pos + 128, 128);
    im->srs_count = npoints;
    // --- upload to GPU if present ---
    if (gpu_ok()) {
        if (hipMalloc(&im->srs_dev, npoints * 64) != hipSuccess) return nullptr;
        if (hipMemcpy(im->srs_dev, im->srs_g1_host.data(), npoints * 64,
                      hipMemcpyHostToDevice) != hipSuccess)
            return nullptr;
    }
    return ctx.release();
}

void rng_ctx_free(RngCtx* ctx) { delete ctx; }

// ---------------- deterministic TEST SRS (product-side) ----------------
// Dev/test deployments need a well-formed SRS without shipping ceremony
// bytes; generating it HERE means the daemon never loads oracle code
// (tier contract: oracle = test infrastructure only).  Byte-identical to
// the test oracle's generator (same tau derivation, same snarkjs subset
// layout parse_ptau_file reads — srs.rs:63-214); production passes real
// ptau bytes to rng_prover_init instead.

namespace {
// minimal host G2 Jacobian over Fq2 (EFD a=0 short-Weierstrass formulas,
// the same shapes as G1Jac) — only used for beta_h = tau*H at generation
struct HG2Jac {
    PFq2 X, Y, Z;
    static HG2Jac from_xy(const PFq2& x, const PFq2& y) { return {x, y, PFq2::one()}; }
    bool is_identity() const { return Z.eq(PFq2::zero()); }
    HG2Jac dbl() const {
        if (is_identity()) return *this;
        PFq2 A = X.sqr(), B = Y.sqr(), C = B.sqr();
        PFq2 D = X.add(B).sqr().sub(A).sub(C);
        D = D.add(D);
        PFq2 E = A.add(A).add(A);
        PFq2 F = E.sqr();
        HG2Jac r;
        r.X = F.sub(D.add(D));
        PFq2 C8 = C.add(C); C8 = C8.add(C8); C8 = C8.add(C8);
        r.Y = E.mul(D.sub(r.X)).sub(C8);
        r.Z = Y.mul(Z); r.Z = r.Z.add(r.Z);
        return r;
    }
    HG2Jac add(const HG2Jac& o) const {
        if (is_identity()) return o;
        if (o.is_identity()) return *this;
        PFq2 Z1Z1 = Z.sqr(), Z2Z2 = o.Z.sqr();
        PFq2 U1 = X.mul(Z2Z2), U2 = o.X.mul(Z1Z1);
        PFq2 S1 = Y.mul(o.Z).mul(Z2Z2), S2 = o.Y.mul(Z).mul(Z1Z1);
        if (U1.eq(U2)) {
            if (S1.eq(S2)) return dbl();
            return {PFq2::one(), PFq2::one(), PFq2::zero()};
        }
        PFq2 H = U2.sub(U1);
        PFq2 I = H.add(H).sqr();
        PFq2 J = H.mul(I);
        PFq2 rr = S2.sub(S1); rr = rr.add(rr);
        PFq2 V = U1.mul(I);
        HG2Jac r;
        r.X = rr.sqr().sub(J).sub(V.add(V));
        PFq2 SJ = S1.mul(J);
        r.Y = rr.mul(V.sub(r.X)).sub(SJ.add(SJ));
        r.Z = Z.add(o.Z).sqr().sub(Z1Z1).sub(Z2Z2).mul(H);
        return r;
    }
};

uint64_t srs_test_ptau_npoints(int power) { return (1ull << power) + 3; }
}  // namespace

uint64_t rng_srs_test_ptau_size(int power) {
    if (power < 2 || power > 20) return 0;
    return 12 + (12 + 44) + (12 + srs_test_ptau_npoints(power) * 64) + (12 + 256);
}

int rng_srs_gen_test_ptau(int power, uint64_t seed, uint8_t* out, size_t out_len) {
    uint64_t need = rng_srs_test_ptau_size(power);
    if (!out || !need || out_len < need) return RNG_ERR_BAD_ARG;
    // tau = keccak256("renegade-amd-srs-tau" || le64(seed)) reduced mod r
    uint8_t msg[28];
    memcpy(msg, "renegade-amd-srs-tau", 20);
    memcpy(msg + 20, &seed, 8);
    uint8_t h32[32];
    keccak256_h(msg, 28, h32);
    u64 limbs[4];
    memcpy(limbs, h32, 32);
    Fr tau = Fr::from_canonical(limbs);
    const uint64_t npoints = srs_test_ptau_npoints(power);
    std::vector<std::array<u64, 4>> scalars(npoints);
    Fr acc = Fr::one();
    for (uint64_t i = 0; i < npoints; ++i) {
        acc.to_canonical(scalars[i].data());
        acc = acc.mul(tau);
    }
    // fixed-base doubling table G_b = 2^b * G
    std::vector<G1Jac> table(256);
    {
        G1Aff g;
        static const u64 gx[4] = G1_GEN_X_MONT, gy[4] = G1_GEN_Y_MONT;
        memcpy(g.x.l, gx, 32);
        memcpy(g.y.l, gy, 32);
        table[0] = G1Jac::from_affine(g);
    }
    for (int j = 1; j < 256; ++j) table[j] = table[j - 1].dbl();
    std::vector<G1Aff> pts(npoints);
    unsigned nthreads = std::thread::hardware_concurrency();
    if (nthreads == 0) nthreads = 1;
    if (nthreads > 64) nthreads = 64;
    std::vector<std::thread> ths;
    std::atomic<uint64_t> next{0};
    for (unsigned t = 0; t < nthreads; ++t)
        ths.emplace_back([&] {
            for (;;) {
                uint64_t lo = next.fetch_add(512);
                if (lo >= npoints) break;
                uint64_t hi = lo + 512 < npoints ? lo + 512 : npoints;
                for (uint64_t i = lo; i < hi; ++i) {
                    G1Jac p = G1Jac::identity();
                    const u64* s = scalars[i].data();
                    for (int b = 0; b < 256; ++b)
                        if ((s[b >> 6] >> (b & 63)) & 1) p = p.add(table[b]);
                    Fq zi = p.Z.inverse();
                    Fq zi2 = zi.sqr();
                    pts[i].x = p.X.mul(zi2);
                    pts[i].y = p.Y.mul(zi2.mul(zi));
                }
            }
        });
    for (auto& th : ths) th.join();
    // beta_h = tau * H (canonical double-and-add, MSB first)
    PFq2 hx, hy;
    {
        static const u64 xc0[4] = G2_GEN_X_C0_MONT, xc1[4] = G2_GEN_X_C1_MONT;
        static const u64 yc0[4] = G2_GEN_Y_C0_MONT, yc1[4] = G2_GEN_Y_C1_MONT;
        memcpy(hx.a.l, xc0, 32);
        memcpy(hx.b.l, xc1, 32);
        memcpy(hy.a.l, yc0, 32);
        memcpy(hy.b.l, yc1, 32);
    }
    u64 tc[4];
    tau.to_canonical(tc);
    HG2Jac hjac = HG2Jac::from_xy(hx, hy);
    HG2Jac bacc{PFq2::one(), PFq2::one(), PFq2::zero()};
    for (int i = 255; i >= 0; --i) {
        bacc = bacc.dbl();
        if ((tc[i >> 6] >> (i & 63)) & 1) bacc = bacc.add(hjac);
    }
    PFq2 bx, by;
    {
        PFq2 zi = bacc.Z.inverse();
        PFq2 zi2 = zi.sqr();
        bx = bacc.X.mul(zi2);
        by = bacc.Y.mul(zi2.mul(zi));
    }
    // --- serialize (layout of srs_to_ptau / parse_ptau_file) ---
    uint8_t* w = out;
    auto put = [&](const void* p, size_t n) { memcpy(w, p, n); w += n; };
    auto put_u32 = [&](uint32_t v) { put(&v, 4); };
    auto put_u64v = [&](uint64_t v) { put(&v, 8); };
    put("ptau", 4);
    put_u32(1);
    put_u32(11);
    put_u32(1);
    put_u64v(44);
    put_u32(32);
    static const u64 qmod[4] = FQ_MODULUS;
    put(qmod, 32);
    put_u32((uint32_t)power);
    put_u32((uint32_t)power);
    put_u32(2);
    put_u64v(npoints * 64);
    for (uint64_t i = 0; i < npoints; ++i) {
        put(pts[i].x.l, 32);
        put(pts[i].y.l, 32);
    }
    put_u32(3);
    put_u64v(256);
    put(hx.a.l, 32);
    put(hx.b.l, 32);
    put(hy.a.l, 32);
    put(hy.b.l, 32);
    put(bx.a.l, 32);
    put(bx.b.l, 32);
    put(by.a.l, 32);
    put(by.b.l, 32);
    return RNG_OK;
}

const void* rng_srs_dev_bases(RngCtx* ctx, uint64_t* count) {
    if (count) *count = ctx->impl.srs_count;
    return ctx->impl.srs_dev;
}

void* rng_dbuf_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    return p;
}
void rng_dbuf_free(void* p) {
    if (p) hipFree(p);
}
int rng_dbuf_upload(void* d, const void* h, size_t bytes) {
    HIP_CHECK(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice));
    return RNG_OK;
}
int rng_dbuf_download(const void* d, void* h, size_t bytes) {
    HIP_CHECK(hipMemcpy(h, (void*)d, bytes, hipMemcpyDeviceToHost));
    return RNG_OK;
}
int rng_device_sync(void) {
    HIP_CHECK(hipDeviceSynchronize());
    return RNG_OK;
}

int rng_ntt_fr_dev(RngCtx* ctx, void* dev_data, uint64_t n, uint64_t batch, int inverse) {
    if (!gpu_ok()) return RNG_ERR_NO_GPU;
    if (!ctx || !dev_data || !ntt_args_ok(n, batch)) return RNG_ERR_BAD_ARG;
    Fr* data = (Fr*)dev_data;
    NttPlan* p = get_plan(&ctx->impl, (uint32_t)n, batch);
    if (!p) return RNG_ERR_HIP;
    if (n <= NTT_SMALL_MAX)
        return ntt_dev_run(&ctx->impl, data, data, (uint32_t)n, batch, inverse);
    int rc = ntt_dev_run(&ctx->impl, data, p->scratch, (uint32_t)n, batch, inverse);
    if (rc != RNG_OK) return rc;
    HIP_CHECK(hipMemcpy(data, p->scratch, n * batch * sizeof(Fr), hipMemcpyDeviceToDevice));
    return RNG_OK;
}

int rng_ntt_fr_dev_oop(RngCtx* ctx, void* dev_in, void* dev_out, uint64_t n,
                       uint64_t batch, int inverse) {
    if (!gpu_ok()) return RNG_ERR_NO_GPU;
    if (!ctx || !dev_in || !dev_out || !ntt_args_ok(n, batch)) return RNG_ERR_BAD_ARG;
    // pass 2 reads contiguous rows and writes strided columns: aliasing races
    if (n > NTT_SMALL_MAX && dev_in == dev_out) return RNG_ERR_BAD_ARG;
    return ntt_dev_run(&ctx->impl, (Fr*)dev_in, (Fr*)dev_out, (uint32_t)n, batch, inverse);
}

int rng_ntt_fr(RngCtx* ctx, uint64_t* data, uint64_t n, uint64_t batch, int inverse) {
    if (!gpu_ok()) return RNG_ERR_NO_GPU;
    if (!ctx || !data || !ntt_args_ok(n, batch)) return RNG_ERR_BAD_ARG;
    size_t bytes = n * batch * sizeof(Fr);
    Fr* d = nullptr;
    HIP_CHECK(hipMalloc(&d, bytes));
    HIP_CHECK(hipMemcpy(d, data, bytes, hipMemcpyHostToDevice));
    NttPlan* p = get_plan(&ctx->impl, (uint32_t)n, batch);
    if (!p) {
        hipFree(d);
        return RNG_ERR_HIP;
    }
    Fr* out = (n <= NTT_SMALL_MAX) ? d : p->scratch;
    int rc = ntt_dev_run(&ctx->impl, d, out, (uint32_t)n, batch, inverse);
    if (rc == RNG_OK) {
        if (hipMemcpy(data, out, bytes, hipMemcpyDeviceToHost) != hipSuccess)
            rc = RNG_ERR_HIP;
    }
    hipFree(d);
    return rc;
}

int rng_msm_g1_dev(RngCtx* ctx, const void* dev_bases, const void* dev_scalars,
                   uint64_t n, uint64_t* out9, int window_c) {
    if (!gpu_ok()) return RNG_ERR_NO_GPU;
    if (!dev_bases || !dev_scalars || !out9 || n == 0) return RNG_ERR_BAD_ARG;
    uint32_t c = window_c > 0 ? (uint32_t)window_c : msm_auto_c(n);
    if (c < 8 || c > 16) return RNG_ERR_BAD_ARG;
    G1Jac res;
    int rc = msm_dev_run(MsmBases::plain((const G1Aff*)dev_bases),
                         (const uint64_t*)dev_scalars, n, c, &res);
    if (rc != RNG_OK) return rc;
    jac_to_affine_record(res, out9);
    return RNG_OK;
}

int rng_msm_srs_batch(RngCtx* ctx, const uint64_t* scalars, uint64_t n, uint32_t B,
                      int window_c, int mode, uint64_t* out9xB) {
    if (!gpu_ok()) return RNG_ERR_NO_GPU;
    if (!ctx || !scalars || !out9xB || n == 0 || B == 0 || mode < 0 || mode > 3)
        return RNG_ERR_BAD_ARG;
    void* ds = nullptr;
    HIP_CHECK(hipMalloc(&ds, (uint64_t)B * n * 32));
    std::vector<G1Jac> res(B);
    int rc = RNG_OK;
    if (hipMemcpy(ds, scalars, (uint64_t)B * n * 32, hipMemcpyHostToDevice) != hipSuccess)
        rc = RNG_ERR_HIP;
    if (rc == RNG_OK)
        rc = msm_srs_run(&ctx->impl, (const uint64_t*)ds, n, B, res.data(), window_c, mode);
    hipFree(ds);
    if (rc != RNG_OK) return rc;
    for (uint32_t b = 0; b < B; ++b) jac_to_affine_record(res[b], out9xB + 9 * b);
    return RNG_OK;
}

int rng_commit_lagrange(RngCtx* ctx, uint64_t n, const uint64_t* evals,
                        const uint64_t* blinders, uint32_t B, int window_c,
                        uint64_t* out9xB) {
    if (!gpu_ok()) return RNG_ERR_NO_GPU;
    if (!ctx || !evals || !out9xB || B == 0 || n < 2 || (n & (n - 1)) ||
        n + 2 > ctx->impl.srs_count || (uint64_t)B * (n + 2) >= (1ull << 31))
        return RNG_ERR_BAD_ARG;
    // pack at stride n + 2 on the host: evaluations, then the two blinders
    std::vector<uint64_t> packed((size_t)B * (n + 2) * 4, 0);
    for (uint32_t b = 0; b < B; ++b) {
        memcpy(&packed[(size_t)b * (n + 2) * 4], evals + (size_t)b * n * 4, n * 32);
        if (blinders)
            memcpy(&packed[((size_t)b * (n + 2) + n) * 4], blinders + (size_t)b * 8, 64);
    }
    void* ds = nullptr;
    HIP_CHECK(hipMalloc(&ds, packed.size() * 8));
    std::vector<G1Jac> res(B);
    int rc = RNG_OK;
    if (hipMemcpy(ds, packed.data(), packed.size() * 8, hipMemcpyHostToDevice) != hipSuccess)
        rc = RNG_ERR_HIP;
    if (rc == RNG_OK)
        rc = msm_lagrange_run(&ctx->impl, n, (const uint64_t*)ds, B, res.data(), window_c,
                              true);
    hipFree(ds);
    if (rc == MSM_LAGRANGE_UNUSABLE) return RNG_ERR_BAD_ARG;
    if (rc != RNG_OK) return rc;
    for (uint32_t b = 0; b < B; ++b) jac_to_affine_record(res[b], out9xB + 9 * b);
    return RNG_OK;
}

int rng_msm_g1(RngCtx* ctx, const uint64_t* bases, const uint64_t* scalars, uint64_t n,
               uint64_t* out9, int window_c) {
    if (!gpu_ok()) return RNG_ERR_NO_GPU;
    if (!bases || !scalars || !out9 || n == 0) return RNG_ERR_BAD_ARG;
    void *db = nullptr, *ds = nullptr;
    HIP_CHECK(hipMalloc(&db, n * 64));
    if (hipMalloc(&ds, n * 32) != hipSuccess) {
        hipFree(db);
        return RNG_ERR_HIP;
    }
    int rc = RNG_OK;
    if (hipMemcpy(db, bases, n * 64, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(ds, scalars, n * 32, hipMemcpyHostToDevice) != hipSuccess)
        rc = RNG_ERR_HIP;
    if (rc == RNG_OK) rc = rng_msm_g1_dev(ctx, db, ds, n, out9, window_c);
    hipFree(db);
    hipFree(ds);
    return rc;
}

#include "circuit_abi.hpp"

// field-mul microbenchmark: returns ms per launch; variant 0 = 64-bit CIOS,
// 1 = 32-bit CIOS; dep = dependent chain
double rng_bench_frmul(int variant, uint32_t blocks, uint32_t iters, int dep,
                       int reps) {
    if (!gpu_ok()) return -1;
    Fr* io = nullptr;
    if (hipMalloc(&io, 1024 * sizeof(Fr)) != hipSuccess) return -1;
    std::vector<Fr> init(1024);
    for (int i = 0; i < 1024; ++i) init[i] = Fr::from_u64(i * 2654435761u + 1);
    hipMemcpy(io, init.data(), 1024 * sizeof(Fr), hipMemcpyHostToDevice);
    auto launch = [&]() {
        if (variant == 0)
            hipLaunchKernelGGL(k_bench_frmul<0>, dim3(blocks), dim3(256), 0, 0, io,
                               iters, dep);
        else if (variant == 1)
            hipLaunchKernelGGL(k_bench_frmul<1>, dim3(blocks), dim3(256), 0, 0, io,
                               iters, dep);
        else
            hipLaunchKernelGGL(k_bench_frmul<2>, dim3(blocks), dim3(256), 0, 0, io,
                               iters, dep);
    };
    launch();
    hipDeviceSynchronize();
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    hipEventRecord(e0, 0);
    for (int r = 0; r < reps; ++r) launch();
    hipEventRecord(e1, 0);
    hipEventSynchronize(e1);
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    hipFree(io);
    return ms / reps;
}

// pairing equality check on raw records (host; for bilinearity tests and
// external use): p1/p2 = 9-u64 G1 affine, q1/q2 = 16-u64 G2 affine.
// Returns 1 if e(p1, q1) == e(p2, q2).
int rng_pairing_check(const uint64_t* p1, const uint64_t* q1, const uint64_t* p2,
                      const uint64_t* q2) {
    if (p1[8] || p2[8]) return -1;  // infinities unsupported here
    Fq p1x, p1y, p2x, p2y;
    memcpy(p1x.l, p1, 32);
    memcpy(p1y.l, p1 + 4, 32);
    memcpy(p2x.l, p2, 32);
    memcpy(p2y.l, p2 + 4, 32);
    PG2 Q1, Q2;
    memcpy(Q1.x.a.l, q1, 32);
    memcpy(Q1.x.b.l, q1 + 4, 32);
    memcpy(Q1.y.a.l, q1 + 8, 32);
    memcpy(Q1.y.b.l, q1 + 12, 32);
    memcpy(Q2.x.a.l, q2, 32);
    memcpy(Q2.x.b.l, q2 + 4, 32);
    memcpy(Q2.y.a.l, q2 + 8, 32);
    memcpy(Q2.y.b.l, q2 + 12, 32);
    return pairing_check_eq(p1x, p1y, Q1, p2x, p2y, Q2) ? 1 : 0;
}

// host G1 addition on 9-u64 affine records (for combining per-rank MSM shard
// results after the RCCL/gloo exchange — SURVEY.md §8e; host-side, tiny)
void rng_g1_add_affine(const uint64_t* a9, const uint64_t* b9, uint64_t* out9) {
    G1Jac s = g1_record_load_jac(a9).add(g1_record_load_jac(b9));
    jac_to_affine_record(s, out9);
}

// host keccak-256 (exported for known-answer tests of the transcript hash)
void rng_keccak256(const uint8_t* data, size_t len, uint8_t* out32) {
    keccak256_h(data, len, out32);
}

// blinder DRBG block i for a given seed (Montgomery limbs out) — lets tests
// pin the oracle/product DRBG spec equality on CPU
void rng_debug_drbg(uint64_t seed, uint32_t n_blocks, uint64_t* out) {
    HostDrbg d(seed);
    for (uint32_t i = 0; i < n_blocks; ++i) {
        Fr b = d.next();
        memcpy(out + 4 * i, b.l, 32);
    }
}

// ---- TurboPlonk prover entry points ----

struct RngProvingKey {
    PlonkPkImpl impl;
};

RngProvingKey* rng_preprocess(RngCtx* ctx, const RngCircuitDesc* desc) {
    if (!gpu_ok() || !ctx || !desc || !desc->selectors || !desc->sigma) return nullptr;
    if (desc->n < 8 || (desc->n & (desc->n - 1))) return nullptr;
    if (desc->n + 3 > ctx->impl.srs_count) return nullptr;  // SRS too small
    auto pk = std::make_unique<RngProvingKey>();
    pk->impl.ctx = &ctx->impl;
    if (plonk_preprocess_impl(&ctx->impl, desc, &pk->impl) != RNG_OK) return nullptr;
    return pk.release();
}

void rng_pk_free(RngProvingKey* pk) { delete pk; }

int rng_prove(RngCtx* ctx, const RngProvingKey* pk, const uint64_t* wires,
              const uint64_t* public_inputs, uint64_t seed, uint64_t* out_proof,
              uint64_t* out_link_hint) {
    if (!gpu_ok()) return RNG_ERR_NO_GPU;
    if (!ctx || !pk || !wires || !out_proof) return RNG_ERR_BAD_ARG;
    if (pk->impl.npub > 0 && !public_inputs) return RNG_ERR_BAD_ARG;
    return plonk_prove_impl(&ctx->impl, pk->impl, 1, (const Fr*)wires,
                            (const Fr*)public_inputs, &seed, out_proof, out_link_hint);
}

int rng_prove_cohort(RngCtx* ctx, const RngProvingKey* pk, uint64_t k,
                     const uint64_t* wires, const uint64_t* public_inputs,
                     const uint64_t* seeds, uint64_t* out_proofs,
                     uint64_t* out_link_hints) {
    if (!gpu_ok()) return RNG_ERR_NO_GPU;
    if (!ctx || !pk || !wires || !seeds || !out_proofs || k == 0 || k > 128)
        return RNG_ERR_BAD_ARG;
    if (pk->impl.npub > 0 && !public_inputs) return RNG_ERR_BAD_ARG;
    return plonk_prove_impl(&ctx->impl, pk->impl, (uint32_t)k, (const Fr*)wires,
                            (const Fr*)public_inputs, seeds, out_proofs, out_link_hints);
}

// host wires (batch x 5 x n) + device tables -> host z (batch x n) through
// perm_product_dev, the prover's own R2 call
static int perm_product_hosted(const uint64_t* wires, const Fr* d_sigma, const Fr* d_wpow,
                               const Fr k5[5], const uint64_t* beta_gamma, uint64_t n,
                               uint64_t batch, uint64_t* out_z) {
    const size_t rows = (size_t)batch * n;
    Fr* d = nullptr;  // wires (5 rows) | num/den workspace (2 rows) | z (rows)
    HIP_CHECK(hipMalloc(&d, 8 * rows * sizeof(Fr)));
    int rc = RNG_OK;
    if (hipMemcpyAsync(d, wires, 5 * rows * sizeof(Fr), hipMemcpyHostToDevice,
                       RNG_STREAM) != hipSuccess)
        rc = RNG_ERR_HIP;
    if (rc == RNG_OK)
        rc = perm_product_dev(d, d_sigma, d_wpow, k5, (const Fr*)beta_gamma, n, batch,
                              d + 5 * rows, d + 7 * rows);
    if (rc == RNG_OK &&
        (hipMemcpyAsync(out_z, d + 7 * rows, rows * sizeof(Fr), hipMemcpyDeviceToHost,
                        RNG_STREAM) != hipSuccess ||
         hipStreamSynchronize(RNG_STREAM) != hipSuccess))
        rc = RNG_ERR_HIP;
    hipFree(d);
    return rc;
}

int rng_perm_product(RngCtx* ctx, const uint64_t* wires, const uint64_t* sigma_evals,
                     const uint64_t* k5, const uint64_t* beta_gamma, uint64_t n,
                     uint64_t batch, uint64_t* out_z) {
    if (!gpu_ok()) return RNG_ERR_NO_GPU;
    if (!ctx || !wires || !sigma_evals || !k5 || !beta_gamma || !out_z || n < 2 ||
        (n & (n - 1)) || n > PERM_MAX_N || batch < 1 || batch > PERM_MAX_BATCH)
        return RNG_ERR_BAD_ARG;
    Fr* t = nullptr;  // sigma (5n) | w^t (n)
    HIP_CHECK(hipMalloc(&t, 6 * n * sizeof(Fr)));
    int rc = RNG_OK;
    if (hipMemcpyAsync(t, sigma_evals, 5 * n * sizeof(Fr), hipMemcpyHostToDevice,
                       RNG_STREAM) != hipSuccess)
        rc = RNG_ERR_HIP;
    if (rc == RNG_OK) {
        hipLaunchKernelGGL(k_pow_table, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0,
                           RNG_STREAM, t + 5 * n, h_fr_root_of_unity((uint32_t)n),
                           (uint64_t)1, n);
        if (hipGetLastError() != hipSuccess) rc = RNG_ERR_HIP;
    }
    if (rc == RNG_OK)
        rc = perm_product_hosted(wires, t, t + 5 * n, (const Fr*)k5, beta_gamma, n, batch,
                                 out_z);
    hipFree(t);
    return rc;
}

int rng_perm_product_pk(RngCtx* ctx, const RngProvingKey* pk, const uint64_t* wires,
                        const uint64_t* beta_gamma, uint64_t batch, int mode,
                        uint64_t* out_z) {
    if (!gpu_ok()) return RNG_ERR_NO_GPU;
    if (!ctx || !pk || !wires || !beta_gamma || !out_z || batch < 1 ||
        batch > PERM_MAX_BATCH || mode < 0 || mode > 2)
        return RNG_ERR_BAD_ARG;
    const PlonkPkImpl& impl = pk->impl;
    const uint64_t n = impl.n;
    bool dev = mode == 1;
    if (mode == 0)
        dev = ProverEnv::on(prover_env().z_device, Z_DEVICE_DEFAULT) && n <= PERM_MAX_N;
    if (dev)
        return perm_product_hosted(wires, impl.sig_evals_dev, impl.wpow_dev, impl.k, beta_gamma, n,
                                   batch, out_z);
    const Fr w = h_fr_root_of_unity((uint32_t)n);
    const Fr* bg = (const Fr*)beta_gamma;
    HostPool::inst().parallel_for((uint32_t)batch, [&](uint32_t p) {
        perm_product_host(impl, w, (const Fr*)wires + (size_t)5 * p * n, bg[2 * p],
                          bg[2 * p + 1], (Fr*)out_z + (size_t)p * n);
    });
    return RNG_OK;
}

int rng_poly_horner(RngCtx* ctx, const uint64_t* polys, uint64_t len, uint64_t group,
                    uint64_t batch, int shared, const uint64_t* points, int mode,
                    uint64_t* out) {
    if (!gpu_ok()) return RNG_ERR_NO_GPU;
    if (!ctx || !polys || !points || !out || !open_shape_ok(len, group, batch, mode))
        return RNG_ERR_BAD_ARG;
    OpenScratch* os = open_scratch_get();
    if (!os) return RNG_ERR_HIP;
    const size_t nseq = (size_t)batch * group;
    const size_t in_elems = (shared ? (size_t)group : nseq) * len;
    const size_t out_elems = mode == 0 ? nseq : nseq * (len - 1);
    Fr* d = nullptr;  // polys | points | out
    HIP_CHECK(hipMalloc(&d, (in_elems + batch + out_elems) * sizeof(Fr)));
    Fr *d_pts = d + in_elems, *d_out = d_pts + batch;
    OpenSeqs q{};
    q.src = d, q.item_stride = shared ? 0 : group * len, q.poly_stride = len;
    q.pts = d_pts, q.pt_stride = 1;
    q.len = (uint32_t)len, q.group = (uint32_t)group;
    q.out = d_out, q.out_item_stride = group * (len - 1), q.out_poly_stride = len - 1;
    int rc = RNG_OK;
    if (hipMemcpyAsync(d, polys, in_elems * sizeof(Fr), hipMemcpyHostToDevice, RNG_STREAM) !=
            hipSuccess ||
        hipMemcpyAsync(d_pts, points, batch * sizeof(Fr), hipMemcpyHostToDevice,
                       RNG_STREAM) != hipSuccess)
        rc = RNG_ERR_HIP;
    if (rc == RNG_OK) rc = horner_dev(os, q, (uint32_t)batch, mode, d_out);
    if (rc == RNG_OK &&
        (hipMemcpyAsync(out, d_out, out_elems * sizeof(Fr), hipMemcpyDeviceToHost,
                        RNG_STREAM) != hipSuccess ||
         hipStreamSynchronize(RNG_STREAM) != hipSuccess))
        rc = RNG_ERR_HIP;
    hipFree(d);
    return rc;
}

int rng_open_pk(RngCtx* ctx, const RngProvingKey* pk, uint64_t k, const uint64_t* polys,
                const uint64_t* points, const uint64_t* scalars, int mode, uint64_t* out_w) {
    if (!gpu_ok()) return RNG_ERR_NO_GPU;
    if (!ctx || !pk || !polys || !points || !scalars || !out_w || k < 1 ||
        k > OPEN_MAX_BATCH || mode < 0 || mode > 2)
        return RNG_ERR_BAD_ARG;
    const PlonkPkImpl& impl = pk->impl;
    const uint64_t n = impl.n;
    const size_t stride = n + 3, item = OPEN_PROOF_POLYS * stride, wlen = 2 * (n + 2);
    bool dev = mode == 1;
    if (mode == 0)
        dev = ProverEnv::on(prover_env().open_device, OPEN_DEVICE_DEFAULT) && n <= OPEN_MAX_N;
    if (dev) {
        if (n > OPEN_MAX_N) return RNG_ERR_BAD_ARG;
        Fr* d = nullptr;  // polys | C | W
        HIP_CHECK(hipMalloc(&d, k * (item + stride + wlen) * sizeof(Fr)));
        Fr *d_c = d + k * item, *d_w = d_c + k * stride;
        int rc = RNG_OK;
        if (hipMemcpyAsync(d, polys, k * item * sizeof(Fr), hipMemcpyHostToDevice,
                           RNG_STREAM) != hipSuccess)
            rc = RNG_ERR_HIP;
        const OpenSrc src{d, item, d + 6 * stride, item};
        if (rc == RNG_OK)
            rc = open_combine_dev(impl, src, (uint32_t)k, (const Fr*)points,
                                  (const Fr*)scalars, d_c, d_w);
        if (rc == RNG_OK &&
            (hipMemcpyAsync(out_w, d_w, k * wlen * sizeof(Fr), hipMemcpyDeviceToHost,
                            RNG_STREAM) != hipSuccess ||
             hipStreamSynchronize(RNG_STREAM) != hipSuccess))
            rc = RNG_ERR_HIP;
        hipFree(d);
        return rc;
    }
    HostPool::inst().parallel_for((uint32_t)k, [&](uint32_t p) {
        const Fr* base = (const Fr*)polys + p * item;
        std::vector<Fr> v[OPEN_PROOF_POLYS];
        const std::vector<Fr>* ps[OPEN_PROOF_POLYS];
        for (int j = 0; j < OPEN_PROOF_POLYS; ++j) {  // true lengths
            const size_t len = (j < 5 || j == 10) ? n + 2 : n + 3;
            v[j].assign(base + j * stride, base + j * stride + len);
            ps[j] = &v[j];
        }
        const Fr* pt = (const Fr*)points + 2 * (size_t)p;
        std::vector<Fr> Wz, Wzw;
        open_host(impl, ps, (const Fr*)scalars + (size_t)OPEN_COUNT * p, pt[0], pt[1], Wz, Wzw);
        Fr* o = (Fr*)out_w + p * wlen;
        memcpy(o, Wz.data(), (n + 2) * sizeof(Fr));
        memcpy(o + (n + 2), Wzw.data(), (n + 2) * sizeof(Fr));
    });
    return RNG_OK;
}

int rng_quotient_pk(RngCtx* ctx, const RngProvingKey* pk, uint64_t k, const uint64_t* polys,
                    const uint64_t* challenges, const uint64_t* blinders, int mode,
                    uint64_t* out_chunks, uint64_t* out_quot) {
    if (!gpu_ok()) return RNG_ERR_NO_GPU;
    if (!ctx || !pk || !polys || !challenges || !out_chunks || k < 1 ||
        k > OPEN_MAX_BATCH || mode < 0 || mode > 2)
        return RNG_ERR_BAD_ARG;
    const PlonkPkImpl& impl = pk->impl;
    const uint64_t n = impl.n, m = 8 * n;
    bool oop = mode == 1;
    if (mode == 0)
        oop = ProverEnv::on(prover_env().open_device, OPEN_DEVICE_DEFAULT) && n <= OPEN_MAX_N;
    if (cohort_scratch_ensure(n, k) != RNG_OK) return RNG_ERR_HIP;
    CohortScratch* cs = tls_cohort_scratch.get();
    std::vector<QuotChal> chs_h(k, quot_chal_fixed(impl));
    const Fr* ch = (const Fr*)challenges;
    for (uint64_t p = 0; p < k; ++p) {
        chs_h[p].beta = ch[3 * p];
        chs_h[p].gamma = ch[3 * p + 1];
        chs_h[p].alpha = ch[3 * p + 2];
        chs_h[p].alpha2 = ch[3 * p + 2].sqr();
    }
    std::vector<Fr> qblind_h(4 * k, Fr::zero());
    if (blinders) memcpy(qblind_h.data(), blinders, 4 * k * sizeof(Fr));
    const size_t chunk_elems = 5 * k * (n + 3);
    HIP_CHECK(hipMemcpyAsync(cs->coset_in, polys, 7 * k * (n + 3) * sizeof(Fr),
                             hipMemcpyHostToDevice, RNG_STREAM));
    int rc = quotient_stage(&ctx->impl, impl, (uint32_t)k, cs, oop, chs_h.data(),
                            qblind_h.data());
    if (rc != RNG_OK) return rc;
    HIP_CHECK(hipMemcpyAsync(out_chunks, cs->stage, chunk_elems * sizeof(Fr),
                             hipMemcpyDeviceToHost, RNG_STREAM));
    if (out_quot)
        HIP_CHECK(hipMemcpyAsync(out_quot, cs->ntt_tmp, k * m * sizeof(Fr),
                                 hipMemcpyDeviceToHost, RNG_STREAM));
    HIP_CHECK(hipStreamSynchronize(RNG_STREAM));  // qblind_h lifetime, outputs complete
    return RNG_OK;
}

// PK introspection for tests / the verifier side
uint64_t rng_pk_n(RngProvingKey* pk) { return pk->impl.n; }
// out: 18 affine records (13 selector comms, 5 sigma comms)
void rng_pk_comms(RngProvingKey* pk, uint64_t* out) {
    for (int s = 0; s < 13; ++s)
        g1_record_store(pk->impl.sel_comms[s], pk->impl.sel_inf[s], out + 9 * s);
    for (int j = 0; j < 5; ++j)
        g1_record_store(pk->impl.sig_comms[j], pk->impl.sig_inf[j], out + 9 * (13 + j));
}

// Full PlonK verifier with the real BN254 pairing (replaces
// PlonkKzgSnark::verify::<SolidityTranscript>, called at traits.rs:1012).
// Host-only CPU path by design: verification is the relayer-side self-check,
// not the GPU proving hot loop.
static G1Jac jac_mul_canon(const G1Jac& p, const Fr& s) {
    u64 e[4];
    s.to_canonical(e);
    G1Jac acc = G1Jac::identity();
    for (int i = 255; i >= 0; --i) {
        acc = acc.dbl();
        if ((e[i >> 6] >> (i & 63)) & 1) acc = acc.add(p);
    }
    return acc;
}

int rng_verify(RngCtx* ctx, const RngProvingKey* pkw, const uint64_t* public_inputs,
               const uint64_t* proof) {
    if (!ctx || !pkw || !proof) return RNG_ERR_BAD_ARG;
    const PlonkPkImpl& pk = pkw->impl;
    const uint64_t n = pk.n;
    if (pk.npub > 0 && !public_inputs) return RNG_ERR_BAD_ARG;
    const Fr* pubs = (const Fr*)public_inputs;
    // --- deserialize proof (layout: include/rng_prover.h) ---
    G1Aff affs[13];
    G1Jac comms[13];
    bool infs[13];
    for (int i = 0; i < 13; ++i) {
        infs[i] = g1_record_load(proof + 9 * i, &affs[i]);
        comms[i] = infs[i] ? G1Jac::identity() : G1Jac::from_affine(affs[i]);
    }
    // Reject malformed proofs BEFORE transcript replay / pairing: the
    // reference's arkworks deserialization enforces curve membership and
    // canonical limb ranges (ark-serialize Validate::Yes on Proof fields);
    // accepting raw records here would feed off-curve points into the Miller
    // loop (invalid-point soundness hazard — ADVICE r01).
    {
        const Fq b3 = Fq::from_u64(3);  // BN254: y^2 = x^3 + 3
        for (int i = 0; i < 13; ++i) {
            if (infs[i]) continue;
            const uint64_t* rec = proof + 9 * i;
            if (Fq::geq_mod(rec) || Fq::geq_mod(rec + 4)) return RNG_ERR_VERIFY;
            const Fq &x = affs[i].x, &y = affs[i].y;
            if (!y.sqr().eq(x.sqr().mul(x).add(b3))) return RNG_ERR_VERIFY;
        }
        for (int i = 0; i < 10; ++i)
            if (Fr::geq_mod(proof + 117 + 4 * i)) return RNG_ERR_VERIFY;
    }
    Fr wire_evals[5], sigma_evals[4], z_shift_eval;
    {
        const uint64_t* e = proof + 117;
        for (int i = 0; i < 5; ++i) memcpy(wire_evals[i].l, e + 4 * i, 32);
        for (int i = 0; i < 4; ++i) memcpy(sigma_evals[i].l, e + 20 + 4 * i, 32);
        memcpy(z_shift_eval.l, e + 36, 32);
    }
    // --- transcript replay ---
    HostTranscript tr;
    h_transcript_init(tr, pk, pubs);
    auto append_comm = [&](int i) { tr.append_g1(affs[i], infs[i]); };
    for (int j = 0; j < 5; ++j) append_comm(j);
    Fr beta = tr.challenge(), gamma = tr.challenge();
    append_comm(5);
    Fr alpha = tr.challenge();
    for (int i = 6; i < 11; ++i) append_comm(i);
    Fr zeta = tr.challenge();
    for (int j = 0; j < 5; ++j) tr.append_fr(wire_evals[j]);
    for (int j = 0; j < 4; ++j) tr.append_fr(sigma_evals[j]);
    tr.append_fr(z_shift_eval);
    Fr v = tr.challenge();
    append_comm(11);
    append_comm(12);
    Fr u = tr.challenge();

    Fr w = h_fr_root_of_unity((uint32_t)n);
    // the provers' own linearization scalars (plonk_rounds.hpp), applied to
    // commitments here
    const LinScalars ls = lin_scalars(pk.k, n, wire_evals, sigma_evals, z_shift_eval, beta,
                                      gamma, alpha, zeta);
    Fr pi_zeta = Fr::zero();
    {
        std::vector<Fr> dens(pk.npub);
        std::vector<Fr> wis(pk.npub);
        Fr wi = Fr::one();
        for (uint64_t i = 0; i < pk.npub; ++i) {
            wis[i] = wi;
            dens[i] = Fr::from_u64(n).mul(zeta.sub(wi));
            wi = wi.mul(w);
        }
        if (pk.npub) {
            dens = hbatch_inverse(dens);
            for (uint64_t i = 0; i < pk.npub; ++i)
                pi_zeta = pi_zeta.add(pubs[i].mul(wis[i]).mul(ls.zh_zeta).mul(dens[i]));
        }
    }
    Fr ED = pi_zeta.neg()
                .add(alpha.mul(z_shift_eval).mul(ls.Bbar).mul(wire_evals[4].add(gamma)))
                .add(alpha.sqr().mul(ls.l1_zeta));

    // [D]; commitments at infinity are skipped
    G1Jac D = G1Jac::identity();
    for (int i = 0; i < 13; ++i)
        if (!pk.sel_inf[i])
            D = D.add(jac_mul_canon(G1Jac::from_affine(pk.sel_comms[i]), ls.sel[i]));
    D = D.add(jac_mul_canon(comms[COMM_Z], ls.z));
    if (!pk.sig_inf[4])
        D = D.add(jac_mul_canon(G1Jac::from_affine(pk.sig_comms[4]), ls.sigma4));
    for (int i = 0; i < 5; ++i)
        D = D.add(jac_mul_canon(comms[COMM_CHUNKS + i], ls.chunk[i]));
    // F, E
    G1Jac F = D;
    Fr E = ED;
    Fr vp = Fr::one();
    for (int j = 0; j < 5; ++j) {
        vp = vp.mul(v);
        F = F.add(jac_mul_canon(comms[j], vp));
        E = E.add(vp.mul(wire_evals[j]));
    }
    for (int j = 0; j < 4; ++j) {
        vp = vp.mul(v);
        if (!pk.sig_inf[j])
            F = F.add(jac_mul_canon(G1Jac::from_affine(pk.sig_comms[j]), vp));
        E = E.add(vp.mul(sigma_evals[j]));
    }
    F = F.add(jac_mul_canon(comms[5], u));
    E = E.add(u.mul(z_shift_eval));

    // P1 = W + u W'; P2 = zeta W + u zeta w W' + F - E*G
    G1Jac Wz = comms[11], Wzw = comms[12];
    G1Jac P1 = Wz.add(jac_mul_canon(Wzw, u));
    G1Jac P2 = jac_mul_canon(Wz, zeta)
                   .add(jac_mul_canon(Wzw, u.mul(zeta).mul(w)))
                   .add(F);
    {
        G1Aff gen;
        static const u64 gx[4] = G1_GEN_X_MONT, gy[4] = G1_GEN_Y_MONT;
        memcpy(gen.x.l, gx, 32);
        memcpy(gen.y.l, gy, 32);
        P2 = P2.add(jac_mul_canon(G1Jac::from_affine(gen), E.neg()));
    }
    // to affine
    auto to_aff = [](const G1Jac& j, Fq& x, Fq& y) {
        Fq zi = j.Z.inverse();
        Fq zi2 = zi.sqr();
        x = j.X.mul(zi2);
        y = j.Y.mul(zi2.mul(zi));
    };
    if (P1.is_identity() || P2.is_identity()) return RNG_ERR_VERIFY;
    Fq p1x, p1y, p2x, p2y;
    to_aff(P1, p1x, p1y);
    to_aff(P2, p2x, p2y);
    // e(P1, [tau]_2) == e(P2, [1]_2)
    PG2 qh, qbh;
    memcpy(qh.x.a.l, ctx->impl.h_g2, 32);
    memcpy(qh.x.b.l, ctx->impl.h_g2 + 4, 32);
    memcpy(qh.y.a.l, ctx->impl.h_g2 + 8, 32);
    memcpy(qh.y.b.l, ctx->impl.h_g2 + 12, 32);
    memcpy(qbh.x.a.l, ctx->impl.beta_h_g2, 32);
    memcpy(qbh.x.b.l, ctx->impl.beta_h_g2 + 4, 32);
    memcpy(qbh.y.a.l, ctx->impl.beta_h_g2 + 8, 32);
    memcpy(qbh.y.b.l, ctx->impl.beta_h_g2 + 12, 32);
    return pairing_check_eq(p1x, p1y, qbh, p2x, p2y, qh) ? RNG_OK : RNG_ERR_VERIFY;
}

// Proof linking (replaces PlonkKzgSnark::link_proofs, called at
// proof_linking/intent_and_balance.rs:66-73).  Spec: oracle/plonk.hpp §link;
// hints are (n+2) wire-0 coefficients + a 9-u64 commitment record (the
// layout rng_prove emits); out = ([q], [W]) as 2 affine records (18 u64).
int rng_link_proofs(RngCtx* ctx, const RngProvingKey* pk, const uint64_t* hint_a,
                    const uint64_t* hint_b, uint64_t group_alignment,
                    uint64_t group_offset, uint64_t group_size,
                    uint64_t* out_link_proof) {
    if (!gpu_ok()) return RNG_ERR_NO_GPU;
    if (!ctx || !pk || !hint_a || !hint_b || !out_link_proof || group_size == 0)
        return RNG_ERR_BAD_ARG;
    const uint64_t n = pk->impl.n;
    const uint64_t hn = n + 2;
    if (prove_scratch_ensure(n) != RNG_OK) return RNG_ERR_HIP;
    std::vector<Fr> diff(hn);
    memcpy(diff.data(), hint_a, hn * sizeof(Fr));
    for (uint64_t i = 0; i < hn; ++i) {
        Fr b;
        memcpy(b.l, hint_b + 4 * i, 32);
        diff[i] = diff[i].sub(b);
    }
    // vanishing polynomial of S = {w_{2^a}^(off+k)} on the alignment grid
    Fr w = h_fr_root_of_unity(1u << group_alignment);
    Fr wi = w.pow_u64(group_offset);
    std::vector<Fr> zs{Fr::one()};
    for (uint64_t i = 0; i < group_size; ++i) {
        std::vector<Fr> nz(zs.size() + 1, Fr::zero());
        for (size_t j = 0; j < zs.size(); ++j) {
            nz[j + 1] = nz[j + 1].add(zs[j]);
            nz[j] = nz[j].sub(zs[j].mul(wi));
        }
        zs = std::move(nz);
        wi = wi.mul(w);
    }
    // q = diff / zs (monic long division)
    std::vector<Fr> q;
    {
        std::vector<Fr> r = diff;
        size_t dd = zs.size() - 1;
        if (r.size() < zs.size()) r.resize(zs.size(), Fr::zero());
        q.assign(r.size() - dd, Fr::zero());
        for (size_t i = r.size(); i-- > dd;) {
            Fr c = r[i];
            q[i - dd] = c;
            if (c.is_zero()) continue;
            for (size_t j = 0; j <= dd; ++j) r[i - dd + j] = r[i - dd + j].sub(zs[j].mul(c));
        }
    }
    G1Aff qc;
    bool qinf;
    if (commit_dev(&ctx->impl, q, &qc, &qinf) != RNG_OK) return RNG_ERR_HIP;
    HostTranscript tr;
    tr.append_u64(group_alignment);
    tr.append_u64(group_offset);
    tr.append_u64(group_size);
    auto append_rec = [&](const uint64_t* rec) {
        G1Aff a;
        bool inf = g1_record_load(rec, &a);
        tr.append_g1(a, inf);
    };
    append_rec(hint_a + 4 * hn);
    append_rec(hint_b + 4 * hn);
    tr.append_g1(qc, qinf);
    Fr eta = tr.challenge();
    Fr zs_eta = hpoly_eval(zs, eta);
    std::vector<Fr> F = diff;
    hpoly_add_scaled(F, q, zs_eta.neg());
    std::vector<Fr> W = hpoly_div_linear(F, eta);
    G1Aff wc;
    bool winf;
    if (commit_dev(&ctx->impl, W, &wc, &winf) != RNG_OK) return RNG_ERR_HIP;
    g1_record_store(qc, qinf, out_link_proof);
    g1_record_store(wc, winf, out_link_proof + 9);
    return RNG_OK;
}

}  // extern "C"
