// C ABI of the MI355X ciphertext-arithmetic backend (see include/alchemy_hip.h) and the element-wise
// kernels around the LDS-resident transforms of kernels_ntt.hpp.
//
// No CPU fallback lives here: every compute entry point needs a gfx950 device and reports
// ALCH_E_NO_DEVICE / ALCH_E_HIP otherwise.  Nothing in this library includes or links oracle/.
#include <hip/hip_runtime.h>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/alchemy_hip.h"
#include "kernels_ntt.hpp"
#include "ring_host.hpp"
#include "gen_host.hpp"
#include "plain_host.hpp"
#include "scratch_plan.hpp"
#include "chacha_stream.hpp"

using namespace alch;

// ------------------------------------------------------------------------------------------------------
// handles
// ------------------------------------------------------------------------------------------------------
// Device tables of the Tensor methods between two indices m | m' (tensor_ext.inc.hpp), cached in the bigger ring.
struct ExtTab {
    u32 d_rel = 0, fibre = 0;
    int32_t* pow_gather = nullptr;     // [n_big]: source position in the small ring, or -1 (embedPow)
    int32_t* coeffs = nullptr;         // [d_rel][n_small]: source position in the big ring (coeffs; row 0 = twacePowDec)
    int32_t* slot_small = nullptr;     // [n_big]: CRT slot of the small ring (embedCRT)
    int32_t* fibres = nullptr;         // [n_small][fibre]: CRT slots of the big ring above a slot of the small ring (twaceCRT)
};

// live streams with a hardware queue of their own (ring option "stream_dedicated"): capped, because the HIP runtime does not survive
// running out of hardware queues (observed: a segmentation fault inside the runtime after ~250 such streams in one process)
static std::atomic<int> g_dedicated_streams{0};
constexpr int MAX_DEDICATED_STREAMS = 32;

struct StreamOwner {
    hipStream_t s;
    int device;
    bool dedicated;
    StreamOwner(hipStream_t s_, int d, bool dedicated_ = false) : s(s_), device(d), dedicated(dedicated_) {}
    ~StreamOwner() {
        if (s) { (void)hipSetDevice(device); (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
        if (dedicated) --g_dedicated_streams;
    }
    StreamOwner(const StreamOwner&) = delete;
    StreamOwner& operator=(const StreamOwner&) = delete;
};

// One device arena of a ring: grown on demand (freed and allocated anew, the old words are not kept), never shrunk.
struct Scratch {
    void* p = nullptr;
    size_t bytes = 0;
    int reserve(size_t need);
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};

struct alch_ring {
    u32 m = 0, n = 0;
    int logn = 0, L = 0, word = 0;            // word = 4 or 8 bytes per residue on the device
    u64 q[MAXL] = {0};
    bool balanced = false;
    bool q30 = false;                          // 32-bit words and every modulus below 2^30 (4q fits a word)
    hipStream_t stream = nullptr;
    // Owner of `stream` when the library created it: shared by every ring that borrowed the stream through alch_ring_share_stream, so
    // the stream outlives the ring that created it for as long as another ring still queues on it (rings are destroyed in any order --
    // a garbage-collected host gives none).  Null when the stream is the caller's (alch_ring_set_stream).
    std::shared_ptr<StreamOwner> stream_owner;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    void* tables = nullptr;                    // all twiddle tables, one allocation
    void* tables_p = nullptr;                  // Plantard forward and inverse constants (32-bit rings) / Shoup pairs (64-bit rings)
    DevRing<u32> d32;
    DevRing<u64> d64;
    Scratch ws_digits;                         // digit scratch, two halves of [chunk][L][n] signed words
    hipStream_t aux = nullptr;                 // second pipeline of ct_mul_relin (odd chunks)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    Scratch ws_in;                             // crt scratch for ALCH_POW_IN (2 * 2*batch elements)
    Scratch ws_host;                           // staging for the host-buffer Tensor methods
    u64* ws_sum = nullptr;                     // checksum accumulator
    size_t chunk = 1024;                       // ciphertexts per (tensor_intt, ks_accum) launch pair
    Scratch ws_full;                           // ct_mul_full scratch: per pipeline digits + key-switched chunk + stash
    hipEvent_t ev_x = nullptr;                 // cross-ring ordering (ext_order)
    Scratch ws_lift;                           // decrypt / error-rate scratch: c(s) of one chunk (+ its crt'd inputs with ALCH_POW_IN)
    Scratch ws_maxd;                           // digit vectors of max |lift|, 8 L bytes per element
    Scratch ws_gauss;                          // alch_buf_gauss_dec on an index with odd primes: the doubles of one chunk of elements
    bool rng_keyed = false;                    // alch_ring_set_rng_key: the samplers that write into this ring draw from ChaCha20 keystreams
    chacha::Key rng_key = {{0}};               // host copy only: it reaches the kernels by value, zeroed on reset and on destroy
    int device = 0;                            // HIP device the ring's streams, tables and buffers live on
    LaunchOpts opts;                           // launch-structure options (alch_ring_set_option)
    bool one_stream = false;
    int nstreams = 2;                          // alch_ct_mul_relin: independent (tensor, key switch) pipelines the chunks rotate over (1 .. 4)
    hipStream_t xs[2] = {nullptr, nullptr};    // pipelines 3 and 4, created on first use
    hipEvent_t ev_xs[2] = {nullptr, nullptr};
    int pipe = 0;                              // alch_ct_mul_relin: 1 = tensor kernels on the aux stream one chunk ahead of the key-switch kernels
    hipEvent_t ev_pa[2] = {nullptr, nullptr}, ev_pb[2] = {nullptr, nullptr};
    unsigned rs_slots = 512;                   // resident workgroups of k_rescale_out (each owns a stash slot)
    size_t scratch_mib = 4096;                 // scratch of the composed (unfused) paths: digits + intermediates of one chunk
                                               // (n = 2^16: 66.3 k op/s at 1 GiB, 73.3 k at 4 GiB, 77.7 k at 16 GiB -- small chunks leave CUs idle)
    alch_buf* scratch = nullptr;               // staging elements of the host-buffer Tensor methods
    // general cyclotomic index (kernel_gen.hpp); two-power rings with n >= 16 keep the radix-16 engine
    bool gen = false;
    bool has_crt = true;                       // false: ring created with alch_ring_create_nocrt (Pow / Dec operations only)
    bool zdom = false;                         // "modulus" 0: the integers, signed 64-bit words
    GenHost gh;
    GenDev<u32> g32;
    GenDev<u64> g64;
    void* gen_tables = nullptr;
    int* d_flag = nullptr;                     // divG failure flag
    std::deque<std::pair<u32, ExtTab>> ext;    // extension tables towards sub-rings of index .first (same moduli)
    std::deque<std::pair<u32, u32*>> autotab;  // general engine: device slot tables of sigma_j, cached per j mod m (alch_buf_automorph)
    Scratch ws_auto;                           // alch_ct_automorph: the permuted ciphertexts of one chunk
    // Free list of small device buffers: alch_buf_alloc / alch_buf_free of single ring elements are the allocation pattern of a
    // device-resident Tensor value (one buffer per `GT` value), and hipMalloc / hipFree cost 50-200 us and synchronise the device.
    // Reuse is stream-ordered: every consumer of a buffer on another ring's stream makes the owner's stream wait for it (ext_order,
    // alch_ct_mod_switch, alch_ct_tunnel, alch_ct_mul_full), so work queued later on the owner's stream may overwrite it.
    std::vector<std::pair<size_t, void*>> pool;                 // (n_elems, device pointer)
    size_t pool_bytes = 0;
    std::mutex pool_mu;                                         // alch_buf_free may come from a finalizer thread (Haskell ForeignPtr)
    // Pinned host staging of small transfers (alch_buf_upload / alch_buf_download of a few ring elements): no pageable-memory copy
    // inside the HIP runtime, no synchronisation on upload, exactly one on download.
    struct Pin { void* p = nullptr; size_t bytes = 0; hipEvent_t ev = nullptr; bool busy = false; };
    Pin pin[4];
    int pin_next = 0;
};

static const size_t POOL_MAX_BUF = (size_t)32 << 20;           // buffers up to 32 MiB are recycled
static const size_t POOL_CAP = (size_t)1 << 30;                // at most 1 GiB parked per ring
static const size_t PIN_MAX = (size_t)8 << 20;                 // transfers up to 8 MiB of int64 go through pinned staging

struct alch_buf {
    alch_ring* ring;
    size_t n_elems;
    void* dptr;
    bool view = false;                         // alch_buf_view: a non-owning alias into another buffer
};

struct alch_tunnel {
    alch_ring* rr;                             // R'_q (input ciphertexts)
    alch_ring* rs;                             // S'_q (hint, output ciphertexts)
    u32 d_rel;                                 // dim of R'/E' = number of E'-coefficients per ring element
    u32 linv_skip_mask;
    int32_t* table;                            // device: [d_rel][n_s] source positions in R', -1 = zero
    void* lin;                                 // device: f' values y_i, [d_rel][L][n_s], CRT basis, Montgomery form
    void* ks;                                  // device: [d_rel * D][2][L][n_s], CRT basis, Montgomery form (D gadget digits)
    int gadget;
    int digits;                                // D: L for TrivGad, sum_i ceil(log2 q_i) for BaseBGad 2
    // E'-level form (null when E' = S' or E' has no general-index ring): an embedded E'-element's CRT over S' is its CRT over E'
    // replicated (embedCRT), so the constant terms' and the digits' transforms run at dimension phi(e') and the products with
    // the linear function / the hints read them through slot_e
    alch_ring* re = nullptr;                   // E'_q, same moduli (owned)
    int32_t* table_e = nullptr;                // device: [d_rel][n_e] source positions in R'
    u32* slot_e = nullptr;                     // device: [n_s] CRT slot of E' behind every CRT slot of S'
    bool pieces_ok = false;                    // every aligned group of four S' slots reads four consecutive, aligned E' slots
    // both rings two-power with m >= 32 (the radix-16 engine): do_tunnel_pow2 -- closed-form index maps, no tables, `re` unused
    bool pow2 = false;
    u32 sh = 0;                                // log2(n_s / n_r) in the up direction (S' slot k reads slot k >> sh of R'), else 0
};

struct alch_hint {
    alch_ring* ring;
    int gadget;
    int digits;
    void* dptr;                                // [digit][2][L][n] words, Montgomery form
};

// ------------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------------
static thread_local std::string g_err;

// element ranges of the C ABI are checked without forming first + count or 2 * batch (a huge argument must not wrap past the check)
static inline bool range_ok(size_t first, size_t count, size_t n) { return count <= n && first <= n - count; }
static inline bool pairs_ok(size_t batch, size_t n) { return batch <= n / 2; }
static bool bytes_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const char *x = reinterpret_cast<const char*>(a), *y = reinterpret_cast<const char*>(b);
    return x < y + nb && y < x + na;
}
// The overlap rule of the element-wise entry points (include/alchemy_hip.h, "Overlapping ranges"): a written range may START where an
// operand's range starts -- every lane reads the words it writes before it writes them, in the vector and in the one-word forms -- and
// any other common byte is a race between lanes: refused.
static bool shifted_overlap(const void* w, size_t nw, const void* r, size_t nr) { return w != r && bytes_overlap(w, nw, r, nr); }
static int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
// No C++ exception leaves the library (include/alchemy_hip.h: "no exceptions across the ABI" -- the callers are C, Haskell's FFI and
// ctypes, where an escaping exception is std::terminate at best): every `extern "C" int` entry point is a function-try-block that
// ends in this handler.  What can throw inside them is host-side allocation (std::vector / std::string / new: std::bad_alloc,
// std::length_error) -- reported as ALCH_E_NOMEM / ALCH_E_INTERNAL with the message in alch_last_error(), never as an abort.
// tests/test_abi_guard.py checks the mechanism through the real ABI (alch_debug_throw) and, lexically, that no entry point lacks it.
static int abi_catch() noexcept {
    int code = ALCH_E_INTERNAL;
    try {
        throw;
    } catch (const std::bad_alloc&) {
        code = ALCH_E_NOMEM;
        try { g_err = "out of host memory (std::bad_alloc)"; } catch (...) {}
    } catch (const std::exception& e) {
        try { g_err = std::string("internal error: ") + e.what(); } catch (...) {}
    } catch (...) {
        try { g_err = "internal error: unknown exception"; } catch (...) {}
    }
    return code;
}
// test hook (not part of the Tensor surface): throws the chosen exception inside a guarded entry point
extern "C" int alch_debug_throw(int kind) try {
    if (kind == 1) throw std::bad_alloc();
    if (kind == 2) throw std::length_error("alch_debug_throw");
    if (kind == 3) throw 42;
    return ALCH_OK;
} catch (...) { return abi_catch(); }

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess)                                                                           \
            return fail(ALCH_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));                 \
    } while (0)

// HIP's current device is per host thread: every entry point first makes the ring's device current, so a host that
// calls from another OS thread (Haskell `safe` FFI calls on a -threaded RTS) still launches on the right GPU.
// Every entry point that touches a ring also takes the lock of the ring's DEVICE for the length of the call (recursive: entry points
// call each other).  A ring's scratch, pools and events are plain members, and calls between rings (embed / twace, tunnels, mul_ over
// three rings) touch several rings at once, so the unit of mutual exclusion is the device: a host that forces tensors from several
// threads (a -threaded Haskell RTS, parallel sparks) gets serialised launches instead of corrupted scratch, and threads that drive
// different GPUs (examples/ringround_multi.cpp) never meet.  alch_buf_free / alch_hint_free / alch_tunnel_free stay outside it: they
// come from finalizer threads and must not wait behind a call that is synchronising the device.
static std::recursive_mutex& device_mutex(int dev) {
    static std::recursive_mutex mu[64];
    return mu[(dev >= 0 && dev < 64) ? dev : 0];
}
#define ALCH_CAT2(a, b) a##b
#define ALCH_CAT(a, b) ALCH_CAT2(a, b)
#ifndef ALCH_NO_DEVICE_LOCK
// How often THIS thread holds the lock of a device (the array mirrors device_mutex).  The helpers that own shared ring state -- the
// scratch element, the extension and automorphism table caches, the pinned slots and ws_host -- take no lock of their own: they run
// inside an entry point's, and refuse to run outside one (ALCH_REQUIRE_DEVICE_LOCK).  A caller that forgot its BIND then fails every
// call, single-threaded ones included, instead of racing once in a while.
static int& device_lock_depth(int dev) {
    static thread_local int depth[64];
    return depth[(dev >= 0 && dev < 64) ? dev : 0];
}
struct DeviceLock {
    std::recursive_mutex& mu;
    int& depth;
    explicit DeviceLock(int dev) : mu(device_mutex(dev)), depth(device_lock_depth(dev)) { mu.lock(); ++depth; }
    ~DeviceLock() { --depth; mu.unlock(); }
    DeviceLock(const DeviceLock&) = delete;
    DeviceLock& operator=(const DeviceLock&) = delete;
};
static inline bool device_lock_held(int dev) { return device_lock_depth(dev) > 0; }
#define ALCH_DEVICE_LOCK(dev) DeviceLock ALCH_CAT(_alch_dev_lock_, __LINE__)(dev)
#else
static inline bool device_lock_held(int) { return true; }
#define ALCH_DEVICE_LOCK(dev) ((void)0)   // tests/test_gpu_threads.py's self-test only (tools/build_variant.sh nolock): never in a product build
#endif
#define ALCH_REQUIRE_DEVICE_LOCK(ringp, who)                                                            \
    do {                                                                                                \
        if (!device_lock_held((ringp)->device))                                                         \
            return fail(ALCH_E_INTERNAL, std::string(who) + ": device lock not held");                  \
    } while (0)
#define BIND(ringp)                                                                                     \
    ALCH_DEVICE_LOCK((ringp)->device);                                                                  \
    do {                                                                                                \
        if (hipSetDevice((ringp)->device) != hipSuccess)                                                \
            return fail(ALCH_E_HIP, "hipSetDevice(" + std::to_string((ringp)->device) + ") failed");    \
    } while (0)

extern "C" const char* alch_last_error(void) { return g_err.c_str(); }
extern "C" uint32_t alch_version(void) { return (1u << 16) | 8u; }   // 1.8: decrypt / errorRate_ on resident batches (alch_ct_error_term, alch_buf_lift, alch_ct_decrypt_lift; kernel_lift.hpp); 1.7: ring tunnels between two-power rings with m >= 32 (do_tunnel_pow2); 1.6: alch_buf_checksum_at, shared streams owned by their last user; 1.5: device-resident Tensor values (alch_buf_tensor_op, alch_buf_copy, alch_ring_share_stream, pooled small buffers, pinned staging), status order of alch_ring_create; 1.4: general cyclotomic indices, l / lInv, real mulG / divG, mulPublic / addPublic, alch_ring_set_option; 1.3: + alch_decompose_base2, BaseBGad hints, alch_ct_mul_full, alch_buf_device_ptr, n = 2^16

// ------------------------------------------------------------------------------------------------------
// element-wise kernels (HBM-bound; 16 B per lane, grid-stride, ~2048 workgroups)
// ------------------------------------------------------------------------------------------------------
__host__ __device__ static inline u64 splitmix64(u64 x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

template <typename W>
__global__ void k_fill_uniform(DevRing<W> R, W* data, size_t words, u64 seed) {
    const size_t n = (size_t)R.n;
    for (size_t w = blockIdx.x * (size_t)blockDim.x + threadIdx.x; w < words; w += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)((w / n) % (size_t)R.L);
        data[w] = (W)(splitmix64(seed + w) % (u64)R.mod[j].q);
    }
}

// Lol's tuple-interleaved int64 (coefficient-major, limb-minor) <-> limb-major device words.
template <typename W, bool TO_DEVICE>
__global__ void k_transpose(DevRing<W> R, W* dev, int64_t* host, size_t elems) {
    const size_t n = (size_t)R.n;
    const size_t L = (size_t)R.L;
    const size_t total = elems * L * n;
    for (size_t w = blockIdx.x * (size_t)blockDim.x + threadIdx.x; w < total; w += (size_t)gridDim.x * blockDim.x) {
        const size_t k = w % n, j = (w / n) % L, e = w / (n * L);
        const size_t h = (e * n + k) * L + j;
        if (TO_DEVICE) dev[w] = (W)(u64)host[h];
        else host[h] = (int64_t)(u64)dev[w];
    }
}

// Position (outer, mid, k) of word w in an [outer][mid < M][k < n] array, advanced by the grid stride with adds and
// carries: n is a run-time value (and not a power of two for a general index), so w / n and w % n per word would be
// 64-bit software divisions -- several hundred instructions against the handful a word of element-wise work needs.
struct Walk3 {
    u32 k, mid; size_t outer;
    u32 sk, smid; size_t souter;
    u32 n, M;
    __device__ Walk3(size_t w0, size_t stride, u32 n_, u32 M_) : n(n_), M(M_) {
        k = (u32)(w0 % n); const size_t t = w0 / n; mid = (u32)(t % M); outer = t / M;
        sk = (u32)(stride % n); const size_t s = stride / n; smid = (u32)(s % M); souter = s / M;
    }
    __device__ void step() {
        k += sk; u32 c = k >= n ? 1u : 0u; k -= c ? n : 0u;
        mid += smid + c; c = mid >= M ? 1u : 0u; mid -= c ? M : 0u;
        outer += souter + c;
    }
};
#define ALCH_WALK(w, total, walk) \
    for (size_t w = blockIdx.x * (size_t)blockDim.x + threadIdx.x; w < (total); w += (size_t)gridDim.x * blockDim.x, walk.step())
#define ALCH_WALK_INIT(n_, M_) Walk3 wk(blockIdx.x * (size_t)blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x, (u32)(n_), (u32)(M_))

// VW consecutive words moved with one access (VW = 16 bytes' worth when the ring dimension is a multiple of it, else 1): the
// element-wise kernels of the general-index path are bound by the number of memory instructions long before HBM.
template <typename W, int VW> struct alignas(sizeof(W) * VW) Pack { W v[VW]; };
#define ALCH_LAUNCH_VW(kern, ringp, items, stream, ...)                                                                         \
    do {                                                                                                                        \
        constexpr int VL_ = Vec4<W>::LANES;                                                                                     \
        if ((ringp)->n % VL_ == 0)                                                                                              \
            hipLaunchKernelGGL((kern<W, VL_>), dim3(ew_grid((items) / VL_)), dim3(256), 0, stream, __VA_ARGS__);                \
        else                                                                                                                    \
            hipLaunchKernelGGL((kern<W, 1>), dim3(ew_grid(items)), dim3(256), 0, stream, __VA_ARGS__);                          \
    } while (0)

enum PwOp { PW_MUL = 0, PW_ADD = 1, PW_SUB = 2 };

// z mod q in [0, q) for a signed z.  |z| < q is the common case (a digit, or a centred residue of a modulus of q's
// size): one conditional add; the software division only runs for the lanes that need it.
template <typename W>
__device__ inline typename Signed<W>::type reduce_signed(typename Signed<W>::type z, W q) {
    typedef typename Signed<W>::type SW;
    if (z < (SW)q && z > -(SW)q) return z < 0 ? z + (SW)q : z;
    SW r = z % (SW)q;
    return r < 0 ? r + (SW)q : r;
}

template <typename W, int OP>
__global__ void k_pointwise(DevRing<W> R, W* dst, const W* a, const W* b, size_t words) {
    const size_t n = (size_t)R.n;
    typedef typename Vec4<W>::type V;
    constexpr int VL = Vec4<W>::LANES;
    const size_t nv = words / VL;
    ALCH_WALK_INIT(n / VL, R.L);
    ALCH_WALK(v, nv, wk) {
        const ModP<W> m = R.mod[wk.mid];
        V x = reinterpret_cast<const V*>(a)[v], y = reinterpret_cast<const V*>(b)[v], z;
#pragma unroll
        for (int e = 0; e < VL; ++e) {
            if (OP == PW_MUL) z[e] = mont_mul(mont_mul(x[e], m.r2, m), y[e], m);
            else if (OP == PW_ADD) z[e] = add_mod(x[e], y[e], m.q);
            else z[e] = sub_mod(x[e], y[e], m.q);
        }
        reinterpret_cast<V*>(dst)[v] = z;
    }
}

// The same, one word per lane: rings whose dimension is not a multiple of the vector width (general indices such as
// m = 9, n = 6), where a 16-byte piece would straddle two limbs.
template <typename W, int OP>
__global__ void k_pointwise_scalar(DevRing<W> R, W* dst, const W* a, const W* b, size_t words) {
    ALCH_WALK_INIT(R.n, R.L);
    ALCH_WALK(w, words, wk) {
        const ModP<W> m = R.mod[wk.mid];
        if (OP == PW_MUL) dst[w] = mont_mul(mont_mul(a[w], m.r2, m), b[w], m);
        else if (OP == PW_ADD) dst[w] = add_mod(a[w], b[w], m.q);
        else dst[w] = sub_mod(a[w], b[w], m.q);
    }
}

// dst = src * s_j (mod q_j); sm[j] = s_j in Montgomery form.  TO_MONT callers pass sm = R^2 mod q.
template <typename W, int VW = 1>
__global__ void k_scale(DevRing<W> R, W* dst, const W* src, size_t words, Scal<W> sm) {
    typedef Pack<W, VW> P;
    ALCH_WALK_INIT(R.n / VW, R.L);
    ALCH_WALK(w, words / VW, wk) {
        P x = reinterpret_cast<const P*>(src)[w];
#pragma unroll
        for (int c = 0; c < VW; ++c) x.v[c] = mont_mul(x.v[c], sm.v[wk.mid], R.mod[wk.mid]);
        reinterpret_cast<P*>(dst)[w] = x;
    }
}

// TrivGad decompose + reduce on one Pow-basis element: digits[i] (limb-major element i) limb j =
// centred(c limb i) mod q_j.
template <typename W>
__global__ void k_decompose_triv(DevRing<W> R, const W* c, W* digits, int balanced) {
    typedef typename Signed<W>::type SW;
    const size_t n = (size_t)R.n;
    const size_t L = (size_t)R.L;
    const size_t total = L * L * n;
    c += (size_t)blockIdx.y * L * n;                       // blockIdx.y: which ring element
    digits += (size_t)blockIdx.y * total;
    ALCH_WALK_INIT(R.n, R.L);
    ALCH_WALK(w, total, wk) {
        const size_t k = wk.k, j = wk.mid, i = wk.outer;
        const W qi = R.mod[i].q, qj = R.mod[j].q;
        const W v = c[i * n + k];
        const SW z = v > ((qi - 1) >> 1) ? (SW)v - (SW)qi : (SW)v;
        SW r;
        if (balanced) r = z < 0 ? z + (SW)qj : z;            // |z| < q_j for every pair of limbs: one add
        else r = reduce_signed<W>(z, qj);
        digits[w] = (W)r;
    }
}

// BaseBGad 2 decompose + reduce of one Pow-basis element.  One thread per (source limb i, coefficient k) walks
// the ceil(log2 q_i) digits (balanced remainder in {0,-1}, top digit absorbs the rest) and writes each one
// reduced into every limb.  first_digit[i] = index of limb i's first digit, kd[i] = its digit count.
// P2: BaseBGad 2^gw, gw >= 2 -- kd[i] = ceil(ceil(log2 q_i) / gw) digits by the closed form of hint_gadget.hpp (pow2_digit).
template <typename W, bool P2 = false>
__global__ void k_decompose_base2(DevRing<W> R, const W* c, W* digits, Scal<u32> first_digit, Scal<u32> kd, u32 D, u32 gw) {
    typedef typename Signed<W>::type SW;
    const size_t n = (size_t)R.n;
    const size_t L = (size_t)R.L;
    c += (size_t)blockIdx.y * L * n;                       // blockIdx.y: which ring element
    digits += (size_t)blockIdx.y * D * L * n;
    ALCH_WALK_INIT(R.n, R.L);
    ALCH_WALK(w, L * n, wk) {
        const size_t k = wk.k, i = wk.mid;
        const W qi = R.mod[i].q;
        const W x = c[i * n + k];
        SW v = x > ((qi - 1) >> 1) ? (SW)x - (SW)qi : (SW)x;
        SW ct = 0;                                       // P2: c_t of the closed form, c_(t+1) = c_t 2^gw + 2^(gw-1)
        for (u32 t = 0; t < kd.v[i]; ++t) {
            SW d;
            if constexpr (P2) {
                d = hintgad::pow2_digit<SW>(v, gw, t, t + 1 == kd.v[i], ct);
                if (t + 1 < kd.v[i]) ct = (SW)(ct << gw) | (SW)((SW)1 << (gw - 1));   // c_k itself may not fit the word
            } else if (t + 1 < kd.v[i]) {
                d = v & 1 ? (SW)-1 : (SW)0;          // v mod 2 in {0,1}; remainder 1 is taken as -1 (2r >= b)
                v = (v - d) / 2;
            } else {
                d = v;
            }
            W* out = digits + (size_t)(first_digit.v[i] + t) * L * n;
            for (size_t j = 0; j < L; ++j) out[j * n + k] = (W)reduce_signed<W>(d, R.mod[j].q);
        }
    }
}

// SymmSHE (*) on linear ciphertexts, element-wise on the CRT basis: c0 = a0 b0 s, c1 = (a0 b1 + a1 b0) s -> out,
// c2 = a1 b1 s -> c2buf (one element per ciphertext).  sr2 = s R^2 (Montgomery).  Used by the BaseBGad key switch.
template <typename W> struct GTab { const W* p[MAXL]; };     // per limb: CRT image of g (Montgomery form), or null

template <typename W, int VW = 1>
__global__ void k_tensor_ew(DevRing<W> R, const W* a, const W* b, W* out, W* c2buf, size_t nct, Scal<W> sr2, int dup,
                            W* c2crt, GTab<W> gt, int c2_compact = 0) {
    // c2_compact: c2buf holds the L - dup limbs of the operands' ring only ([ct][L - dup][n]): the added limbs of c2 are zero and
    // neither their crtInv nor their digits are ever computed
    // gt: general index -- SymmSHE's (*) applies mulG to every product coefficient (mulGCRT = pointwise product with the
    // CRT image of g); all-null for a two-power index, where g = 1
    // c2crt != null: a second copy of c2 that stays in the CRT basis (the diagonal digits of the key switch)
    // R: the ring of out / c2buf (L limbs); a, b live on its last L - dup limbs; the dup leading limbs of the
    // results are zero (modSwitch up: Rescale b -> (a,b), its q_a factor folded into sr2 by the host)
    typedef Pack<W, VW> P;
    const size_t n = (size_t)R.n;
    const size_t Ln = (size_t)R.L * n, Lsn = (size_t)(R.L - dup) * n, off = (size_t)dup * n;
    ALCH_WALK_INIT(R.n / VW, R.L);
    ALCH_WALK(w, nct * Ln / VW, wk) {
        const size_t ct = wk.outer, rem = (size_t)wk.mid * n + (size_t)wk.k * VW;
        P c0, c1, c2;
        if (rem < off) {
#pragma unroll
            for (int c = 0; c < VW; ++c) { c0.v[c] = 0; c1.v[c] = 0; c2.v[c] = 0; }
        } else {
            const size_t rs = rem - off, js = wk.mid - (u32)dup;
            const ModP<W> m = R.mod[wk.mid];
            const P a0 = *reinterpret_cast<const P*>(a + 2 * ct * Lsn + rs), a1 = *reinterpret_cast<const P*>(a + (2 * ct + 1) * Lsn + rs);
            const P b0 = *reinterpret_cast<const P*>(b + 2 * ct * Lsn + rs), b1 = *reinterpret_cast<const P*>(b + (2 * ct + 1) * Lsn + rs);
            const W* g = gt.p[wk.mid];
            P gv;
            if (g) gv = *reinterpret_cast<const P*>(g + (size_t)wk.k * VW);
#pragma unroll
            for (int c = 0; c < VW; ++c) {
                const W x0 = mont_mul(a0.v[c], sr2.v[js], m), x1 = mont_mul(a1.v[c], sr2.v[js], m);      // a s R
                W c0v = mont_mul(b0.v[c], x0, m);
                W c1v = add_mod(mont_mul(b1.v[c], x0, m), mont_mul(b0.v[c], x1, m), m.q);
                W c2v = mont_mul(b1.v[c], x1, m);
                if (g) { c0v = mont_mul(c0v, gv.v[c], m); c1v = mont_mul(c1v, gv.v[c], m); c2v = mont_mul(c2v, gv.v[c], m); }
                c0.v[c] = c0v; c1.v[c] = c1v; c2.v[c] = c2v;
            }
        }
        *reinterpret_cast<P*>(out + 2 * ct * Ln + rem) = c0;
        *reinterpret_cast<P*>(out + (2 * ct + 1) * Ln + rem) = c1;
        if (!c2_compact) *reinterpret_cast<P*>(c2buf + ct * Ln + rem) = c2;
        else if (rem >= off) *reinterpret_cast<P*>(c2buf + ct * Lsn + (rem - off)) = c2;
        if (c2crt) *reinterpret_cast<P*>(c2crt + ct * Ln + rem) = c2;
    }
}

// SymmSHE (*) as a step of its own (alch_ct_mul): the quadratic ciphertext of slot ct goes straight to elements (3 ct, 3 ct + 1, 3 ct + 2)
// of out = (c0, c1, c2) -- the layout alch_ct_error_term reads for degree 2.  a, b and out live on one ring; sr2 = s R^2, gt as above.
template <typename W, int VW = 1>
__global__ void k_ct_tensor3(DevRing<W> R, const W* a, const W* b, W* out, size_t nct, Scal<W> sr2, GTab<W> gt) {
    typedef Pack<W, VW> P;
    const size_t n = (size_t)R.n, Ln = (size_t)R.L * n;
    ALCH_WALK_INIT(R.n / VW, R.L);
    ALCH_WALK(w, nct * Ln / VW, wk) {
        const size_t ct = wk.outer, rem = (size_t)wk.mid * n + (size_t)wk.k * VW;
        const ModP<W> m = R.mod[wk.mid];
        const W s = sr2.v[wk.mid];
        const P a0 = *reinterpret_cast<const P*>(a + 2 * ct * Ln + rem), a1 = *reinterpret_cast<const P*>(a + (2 * ct + 1) * Ln + rem);
        const P b0 = *reinterpret_cast<const P*>(b + 2 * ct * Ln + rem), b1 = *reinterpret_cast<const P*>(b + (2 * ct + 1) * Ln + rem);
        const W* g = gt.p[wk.mid];
        P gv, c0, c1, c2;
        if (g) gv = *reinterpret_cast<const P*>(g + (size_t)wk.k * VW);
#pragma unroll
        for (int c = 0; c < VW; ++c) {
            const W x0 = mont_mul(a0.v[c], s, m), x1 = mont_mul(a1.v[c], s, m);                          // a s R
            W c0v = mont_mul(b0.v[c], x0, m);
            W c1v = add_mod(mont_mul(b1.v[c], x0, m), mont_mul(b0.v[c], x1, m), m.q);
            W c2v = mont_mul(b1.v[c], x1, m);
            if (g) { c0v = mont_mul(c0v, gv.v[c], m); c1v = mont_mul(c1v, gv.v[c], m); c2v = mont_mul(c2v, gv.v[c], m); }
            c0.v[c] = c0v; c1.v[c] = c1v; c2.v[c] = c2v;
        }
        W* o = out + 3 * ct * Ln + rem;
        *reinterpret_cast<P*>(o) = c0;
        *reinterpret_cast<P*>(o + Ln) = c1;
        *reinterpret_cast<P*>(o + 2 * Ln) = c2;
    }
}

// SymmSHE (+), (-) and negate on operands that are not aligned (alch_ct_add): out_i = fa * a_i + fb * b_i for every component i, with
// one combined factor per operand, f = g^d * s -- the g-power that brings the operand to the common k and the per-limb scalar that
// carries its encoding change and Z_p scalar.  sa, sb = s R (Montgomery; read only when bit 0 / bit 1 of `scaled`
// is set), gt = the CRT image of g in Montgomery form (all-null where g = 1: the powers are then ignored), ga, gb = the powers.
// DA, DB = the operands' degrees, DB = 0: no second operand (negate, mulG or an encoding change of a whole ciphertext).  A
// ciphertext of degree d is elements (d + 1) ct .. (d + 1) ct + d; out has degree max(DA, DB), and a c2 that only one operand has
// is scaled and stored, never summed with a zero.  Every word of out is read (from whichever operand out aliases) and written by
// the same lane, so out may be a or b when that operand has the result's degree.
template <typename W>
__device__ inline W ct_add_factor(W gw, u32 d, bool has_s, W s, const ModP<W>& m) {
    if (d == 0) return s;                                   // the caller asks only when d > 0 or has_s
    W f = gw;                                               // g R
    for (u32 i = 1; i < d; ++i) f = mont_mul(f, gw, m);     // g^d R
    return has_s ? mont_mul(f, s, m) : f;                   // g^d s R
}

template <typename W, int VW, int DA, int DB>
__global__ void k_ct_add(DevRing<W> R, const W* a, const W* b, W* out, size_t nct, Scal<W> sa, Scal<W> sb, GTab<W> gt, u32 ga, u32 gb,
                         u32 scaled) {
    typedef Pack<W, VW> P;
    constexpr int DO = DA > DB ? DA : DB, DS = DA < DB ? DA : DB;
    const size_t n = (size_t)R.n, Ln = (size_t)R.L * n;
    ALCH_WALK_INIT(R.n / VW, R.L);
    ALCH_WALK(w, nct * Ln / VW, wk) {
        const size_t ct = wk.outer, rem = (size_t)wk.mid * n + (size_t)wk.k * VW;
        const ModP<W> m = R.mod[wk.mid];
        const W* g = (ga | gb) ? gt.p[wk.mid] : nullptr;
        P gv;
        if (g) gv = *reinterpret_cast<const P*>(g + (size_t)wk.k * VW);
        const u32 da = g ? ga : 0u, db = g ? gb : 0u;
        const bool has_sa = (scaled & 1u) != 0, has_sb = (scaled & 2u) != 0;
        P x[DO + 1];
        const W* pa = a + (size_t)(DA + 1) * ct * Ln + rem;
#pragma unroll
        for (int i = 0; i <= DA; ++i) x[i] = *reinterpret_cast<const P*>(pa + (size_t)i * Ln);
        if (da || has_sa) {
#pragma unroll
            for (int c = 0; c < VW; ++c) {
                const W f = ct_add_factor<W>(g ? gv.v[c] : (W)0, da, has_sa, sa.v[wk.mid], m);
#pragma unroll
                for (int i = 0; i <= DA; ++i) x[i].v[c] = mont_mul(x[i].v[c], f, m);
            }
        }
        if constexpr (DB > 0) {
            P y[DB + 1];
            const W* pb = b + (size_t)(DB + 1) * ct * Ln + rem;
#pragma unroll
            for (int i = 0; i <= DB; ++i) y[i] = *reinterpret_cast<const P*>(pb + (size_t)i * Ln);
            if (db || has_sb) {
#pragma unroll
                for (int c = 0; c < VW; ++c) {
                    const W f = ct_add_factor<W>(g ? gv.v[c] : (W)0, db, has_sb, sb.v[wk.mid], m);
#pragma unroll
                    for (int i = 0; i <= DB; ++i) y[i].v[c] = mont_mul(y[i].v[c], f, m);
                }
            }
#pragma unroll
            for (int i = 0; i <= DS; ++i)
#pragma unroll
                for (int c = 0; c < VW; ++c) x[i].v[c] = add_mod(x[i].v[c], y[i].v[c], m.q);
#pragma unroll
            for (int i = DA + 1; i <= DB; ++i) x[i] = y[i];
        }
        W* o = out + (size_t)(DO + 1) * ct * Ln + rem;
#pragma unroll
        for (int i = 0; i <= DO; ++i) *reinterpret_cast<P*>(o + (size_t)i * Ln) = x[i];
    }
}

// The way into keySwitchQuadCirc as a step of its own (alch_ct_key_switch_quad): the components of `nct` quadratic ciphertexts
// (elements 3 ct ..) times toMSD's scalar (sm = s R; scale = 0: s = 1, plain copies): (c0, c1) -> pair [ct][2], c2 -> c2a [ct] and,
// when given, a second copy c2b (the one that stays in the CRT basis).
template <typename W, int VW = 1>
__global__ void k_ct_split3(DevRing<W> R, const W* in, W* pair, W* c2a, W* c2b, size_t nct, Scal<W> sm, int scale) {
    typedef Pack<W, VW> P;
    const size_t n = (size_t)R.n, Ln = (size_t)R.L * n;
    ALCH_WALK_INIT(R.n / VW, R.L);
    ALCH_WALK(w, nct * Ln / VW, wk) {
        const size_t ct = wk.outer, rem = (size_t)wk.mid * n + (size_t)wk.k * VW;
        const W* i = in + 3 * ct * Ln + rem;
        P c0 = *reinterpret_cast<const P*>(i), c1 = *reinterpret_cast<const P*>(i + Ln), c2 = *reinterpret_cast<const P*>(i + 2 * Ln);
        if (scale) {
            const ModP<W> m = R.mod[wk.mid];
            const W s = sm.v[wk.mid];
#pragma unroll
            for (int c = 0; c < VW; ++c) { c0.v[c] = mont_mul(c0.v[c], s, m); c1.v[c] = mont_mul(c1.v[c], s, m); c2.v[c] = mont_mul(c2.v[c], s, m); }
        }
        *reinterpret_cast<P*>(pair + 2 * ct * Ln + rem) = c0;
        *reinterpret_cast<P*>(pair + (2 * ct + 1) * Ln + rem) = c1;
        *reinterpret_cast<P*>(c2a + ct * Ln + rem) = c2;
        if (c2b) *reinterpret_cast<P*>(c2b + ct * Ln + rem) = c2;
    }
}

// keySwitchQuadCirc's inner product for a many-digit gadget: out_c += sum_d digit_d * hint_{d,c} (CRT basis).
// digits: [ct][D][L][n]; hint: [D][2][L][n] in Montgomery form.
template <typename W>
__global__ void k_hint_mac(DevRing<W> R, W* out, const W* digits, const W* hint, size_t nct, u32 D, const W* diag = nullptr,
                           u32 grp = 0, u32 hskip = 0, const u32* slot_e = nullptr, u32 n_d = 0) {
    // slot_e != null (tunnel, E'-level transforms): the digits are CRT vectors of dimension n_d over E'; slot s of S' reads
    // entry slot_e[s] (embedCRT replication).
    // hskip != 0 (tunnel on ciphertexts `hskip` limbs below the hint's ring): the digits come in groups of grp = L - hskip
    // source limbs per embedded coefficient and the hint rows of the absent (zero) limbs are skipped: digit d uses hint row
    // d + (d / grp + 1) * hskip.
    // diag != null (TrivGad, D = L): digit d reduced into its own limb d is c2's limb d itself, read from the CRT-basis
    // copy `diag` [ct][L][n] instead of a transformed digit (those slots of `digits` are never written).
    // One thread owns one (limb, slot) of TILE consecutive ciphertexts, so a hint word is loaded once per TILE
    // products (the hint is the larger stream for a many-digit gadget: 2 D words against D per ciphertext).
    constexpr int TILE = 4;          // 8 was measured slower (HomomRLWR pipeline 18.6 k -> 17.3 k/s): fewer, longer threads
    const size_t n = (size_t)R.n;
    const size_t Ln = (size_t)R.L * n;
    const size_t ntile = (nct + TILE - 1) / TILE;
    ALCH_WALK_INIT(R.n, R.L);
    ALCH_WALK(w, ntile * Ln, wk) {
        const size_t ct0 = wk.outer * TILE, rem = (size_t)wk.mid * n + wk.k;
        const u32 limb = wk.mid;
        const ModP<W> m = R.mod[limb];
        W acc0[TILE], acc1[TILE];
#pragma unroll
        for (int c = 0; c < TILE; ++c) {
            const bool live = ct0 + c < nct;
            acc0[c] = live ? out[2 * (ct0 + c) * Ln + rem] : (W)0;
            acc1[c] = live ? out[(2 * (ct0 + c) + 1) * Ln + rem] : (W)0;
        }
        for (u32 d = 0; d < D; ++d) {
            const u32 hd = hskip ? d + (d / grp + 1) * hskip : d;
            const W h0 = hint[(size_t)(2 * hd) * Ln + rem], h1 = hint[(size_t)(2 * hd + 1) * Ln + rem];
#pragma unroll
            for (int c = 0; c < TILE; ++c) {
                if (ct0 + c >= nct) continue;
                const size_t ct = ct0 + c;
                const W x = slot_e ? digits[((ct * (size_t)D + d) * R.L + limb) * (size_t)n_d + slot_e[wk.k]]
                                   : (diag && hd == limb) ? diag[ct * Ln + rem] : digits[(ct * (size_t)D + d) * Ln + rem];
                acc0[c] = add_mod(acc0[c], mont_mul(x, h0, m), m.q);
                acc1[c] = add_mod(acc1[c], mont_mul(x, h1, m), m.q);
            }
        }
#pragma unroll
        for (int c = 0; c < TILE; ++c) {
            if (ct0 + c >= nct) continue;
            out[2 * (ct0 + c) * Ln + rem] = acc0[c];
            out[(2 * (ct0 + c) + 1) * Ln + rem] = acc1[c];
        }
    }
}

// The same with 16-byte accesses: a thread owns one piece of VL consecutive slots of TILE ciphertexts (n a multiple of VL).
// The one-word form moved 2.4 TB/s in the HomomRLWR pipeline -- bound by the number of memory instructions, not by HBM.
template <typename W, int TILE>
__global__ void k_hint_mac_v(DevRing<W> R, W* out, const W* digits, const W* hint, size_t nct, u32 D, const W* diag, u32 grp, u32 hskip,
                             const u32* slot_e, u32 n_d) {
    typedef typename Vec4<W>::type V;
    // TILE ciphertexts share every hint piece.  Measured on the HomomRLWR pipeline with E'-level digits (small vectors served by
    // L2, the hint rows being what comes from HBM): TILE 2 -> 29.3 k, 4 -> 29.5 k, 8 -> 23.5 k ringRounds/s
    constexpr int VL = Vec4<W>::LANES;
    const size_t n = (size_t)R.n;
    const size_t Ln = (size_t)R.L * n;
    const size_t ntile = (nct + TILE - 1) / TILE;
    const size_t nv = n / VL;                                  // 16-byte pieces per limb-polynomial
    ALCH_WALK_INIT(nv, R.L);
    ALCH_WALK(w, ntile * (size_t)R.L * nv, wk) {
        const size_t ct0 = wk.outer * TILE, rem = (size_t)wk.mid * n + (size_t)wk.k * VL;
        const u32 limb = wk.mid;
        const W q = R.mod[limb].q, qni = R.mod[limb].qni;
        // E'-level digits: the VL slots of this piece read entries se[0..VL) of the small CRT vector; they are consecutive and
        // 16-byte aligned whenever the innermost prime-power factor of s' divides e' with the same exponent (every hop of the
        // reference), else gathered one by one
        u32 se[VL];
        bool piece = false;
        if (slot_e) {
#pragma unroll
            for (int e = 0; e < VL; ++e) se[e] = slot_e[(size_t)wk.k * VL + e];
            piece = (se[0] % VL == 0);
#pragma unroll
            for (int e = 1; e < VL; ++e) piece = piece && se[e] == se[0] + (u32)e;
        }
        V acc0[TILE], acc1[TILE];
#pragma unroll
        for (int c = 0; c < TILE; ++c) {
            const size_t ct = ct0 + c < nct ? ct0 + c : ct0;   // a dead lane of the tile recomputes ciphertext ct0 and stores nothing
            acc0[c] = *reinterpret_cast<const V*>(out + 2 * ct * Ln + rem);
            acc1[c] = *reinterpret_cast<const V*>(out + (2 * ct + 1) * Ln + rem);
        }
        for (u32 d = 0; d < D; ++d) {
            const u32 hd = hskip ? d + (d / grp + 1) * hskip : d;
            const V h0 = *reinterpret_cast<const V*>(hint + (size_t)(2 * hd) * Ln + rem);
            const V h1 = *reinterpret_cast<const V*>(hint + (size_t)(2 * hd + 1) * Ln + rem);
            const bool dg = diag && hd == limb;
#pragma unroll
            for (int c = 0; c < TILE; ++c) {
                const size_t ct = ct0 + c < nct ? ct0 + c : ct0;
                V x;
                if (slot_e) {
                    const W* dv = digits + ((ct * (size_t)D + d) * R.L + limb) * (size_t)n_d;
                    if (piece) x = *reinterpret_cast<const V*>(dv + se[0]);
                    else {
#pragma unroll
                        for (int e = 0; e < VL; ++e) x[e] = dv[se[e]];
                    }
                } else {
                    x = dg ? *reinterpret_cast<const V*>(diag + ct * Ln + rem)
                           : *reinterpret_cast<const V*>(digits + (ct * (size_t)D + d) * Ln + rem);
                }
#pragma unroll
                for (int e = 0; e < VL; ++e) {
                    acc0[c][e] = csub((W)(acc0[c][e] + csub(mont_mul_lazy(x[e], h0[e], q, qni), q)), q);
                    acc1[c][e] = csub((W)(acc1[c][e] + csub(mont_mul_lazy(x[e], h1[e], q, qni), q)), q);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < TILE; ++c) {
            if (ct0 + c >= nct) continue;
            *reinterpret_cast<V*>(out + 2 * (ct0 + c) * Ln + rem) = acc0[c];
            *reinterpret_cast<V*>(out + (2 * (ct0 + c) + 1) * Ln + rem) = acc1[c];
        }
    }
}

// The E'-level form of k_hint_mac_v on its own (tunnels whose digits were transformed at dimension phi(e'), every 16-byte piece of S'
// slots reading one aligned piece of the small vector: alch_tunnel::pieces_ok): without the other forms' address paths the kernel
// needs far fewer registers than k_hint_mac_v's 128 + scratch.
template <typename W, int TILE>
__global__ void k_hint_mac_e(DevRing<W> R, W* out, const W* digits, const W* hint, size_t nct, u32 D, u32 grp, u32 hskip,
                             const u32* slot_e, u32 n_d) {
    typedef typename Vec4<W>::type V;
    constexpr int VL = Vec4<W>::LANES;
    const size_t n = (size_t)R.n;
    const size_t Ln = (size_t)R.L * n;
    const size_t ntile = (nct + TILE - 1) / TILE;
    const size_t nv = n / VL;
    ALCH_WALK_INIT(nv, R.L);
    ALCH_WALK(w, ntile * (size_t)R.L * nv, wk) {
        const size_t ct0 = wk.outer * TILE, rem = (size_t)wk.mid * n + (size_t)wk.k * VL;
        const u32 limb = wk.mid;
        const W q = R.mod[limb].q, qni = R.mod[limb].qni;
        const u32 se = slot_e[(size_t)wk.k * VL];
        V acc0[TILE], acc1[TILE];
        const W* dv[TILE];
#pragma unroll
        for (int c = 0; c < TILE; ++c) {
            const size_t ct = ct0 + c < nct ? ct0 + c : ct0;   // a dead lane of the tile recomputes ciphertext ct0 and stores nothing
            acc0[c] = *reinterpret_cast<const V*>(out + 2 * ct * Ln + rem);
            acc1[c] = *reinterpret_cast<const V*>(out + (2 * ct + 1) * Ln + rem);
            dv[c] = digits + (ct * (size_t)D * R.L + limb) * (size_t)n_d + se;
        }
        const size_t dstep = (size_t)R.L * n_d;
        for (u32 d = 0; d < D; ++d) {
            const u32 hd = hskip ? d + (d / grp + 1) * hskip : d;
            const V h0 = *reinterpret_cast<const V*>(hint + (size_t)(2 * hd) * Ln + rem);
            const V h1 = *reinterpret_cast<const V*>(hint + (size_t)(2 * hd + 1) * Ln + rem);
#pragma unroll
            for (int c = 0; c < TILE; ++c) {
                const V x = *reinterpret_cast<const V*>(dv[c] + (size_t)d * dstep);
#pragma unroll
                for (int e = 0; e < VL; ++e) {
                    acc0[c][e] = csub((W)(acc0[c][e] + csub(mont_mul_lazy(x[e], h0[e], q, qni), q)), q);
                    acc1[c][e] = csub((W)(acc1[c][e] + csub(mont_mul_lazy(x[e], h1[e], q, qni), q)), q);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < TILE; ++c) {
            if (ct0 + c >= nct) continue;
            *reinterpret_cast<V*>(out + 2 * (ct0 + c) * Ln + rem) = acc0[c];
            *reinterpret_cast<V*>(out + (2 * (ct0 + c) + 1) * Ln + rem) = acc1[c];
        }
    }
}

// Round 4: the tunnel's hint inner product with lazy 64-bit accumulation, and evalLin's constant term as its starting value.
//
// k_hint_mac_e spends 7 VALU instructions per (slot, digit, hint row): a Montgomery product (3), its conditional subtraction, the
// addition and the sum's conditional subtraction.  On the hops whose digits were transformed in E' (every S' slot re-reads an E'
// entry but multiplies it by its OWN hint word) that made the kernel VALU-bound: 5.7 10^11 slot-piece-digits/s x 56 lane
// instructions is 82 % of the chip's integer issue rate on Tunnel.hs's first hop, while the digits arrive at 2.3 TB/s, half of
// what a copy moves (profiles/r04_tunnel_hs_kernel_stats_before.csv).  Here a group of K products is summed in 64 bits and reduced
// once: with t the running sum in [0, 2q), acc = t * (R mod q) + sum_{K} x h stays below q 2^32 as long as (K + 2) q < 2^32, and one
// Montgomery reduction of acc is again the running sum in [0, 2q).  K = floor((2^32 - 1) / q) - 2: 5 for Tunnel.hs's moduli
// (examples/Tunnel.hs:34-39, ~2^29), 3 for HomomRLWR's three rounding moduli, 0 for its 30.5-bit ones -- those limbs keep the
// product-at-a-time form.  Per (slot, digit, row): (K + 1 + 3) / K instructions = 1.8 at K = 5.  Same residues: the sum is the
// same element of Z_q, reduced to [0, q) at the end.
// lin != null: c0' starts from sum_i crt(x0_i) y_i (evalLin on the constant term, what k_tunnel_lin computed into `out` in a pass
// of its own) and c1' from zero -- one kernel launch, one write and one read of the output ciphertexts less per tunnel.
template <int TILE>
__global__ void __launch_bounds__(256) k_tunnel_mac_e(DevRing<u32> R, u32* out, const u32* digits, const u32* hint, size_t nct, u32 D, u32 grp, u32 hskip,
                                                      const u32* slot_e, u32 n_d, const u32* x0crt, const u32* lin, u32 d_rel, u32 Lx, u32 xoff) {
    typedef u32 W;
    typedef typename Vec4<W>::type V;
    constexpr int VL = 4;
    const size_t n = (size_t)R.n;
    const size_t Ln = (size_t)R.L * n;
    const size_t ntile = (nct + TILE - 1) / TILE;
    const size_t nv = n / VL;
    ALCH_WALK_INIT(nv, R.L);
    ALCH_WALK(w, ntile * (size_t)R.L * nv, wk) {
        const size_t ct0 = wk.outer * TILE, rem = (size_t)wk.mid * n + (size_t)wk.k * VL;
        const u32 limb = wk.mid;
        const W q = R.mod[limb].q, qni = R.mod[limb].qni;
        const u32 se = slot_e ? slot_e[(size_t)wk.k * VL] : wk.k * (u32)VL;      // no slot table: the digits were transformed in S' itself
        const u32 K = lazy_group(q);                            // (K + 2) q < 2^32
        const bool lazy = K >= 2;
        const W r1 = lazy ? R.mod[limb].r1 : (W)1;            // not lazy: the accumulators hold the running sum itself, in [0, q)
        u64 a0[TILE][VL], a1[TILE][VL];
        const W* dv[TILE];
        // starting values, as acc = value * (R mod q) < q^2
#pragma unroll
        for (int c = 0; c < TILE; ++c) {
            const size_t ct = ct0 + c < nct ? ct0 + c : ct0;   // a dead lane of the tile recomputes ciphertext ct0 and stores nothing
            dv[c] = digits + (ct * (size_t)D * R.L + limb) * (size_t)n_d + se;
            if (lin) {
#pragma unroll
                for (int e = 0; e < VL; ++e) { a0[c][e] = 0; a1[c][e] = 0; }
                if (limb >= xoff) {
                    for (u32 i = 0; i < d_rel; ++i) {
                        const V x = *reinterpret_cast<const V*>(x0crt + ((ct * d_rel + i) * (size_t)Lx + (limb - xoff)) * (size_t)n_d + se);
                        const V y = *reinterpret_cast<const V*>(lin + (size_t)i * Ln + rem);
#pragma unroll
                        for (int e = 0; e < VL; ++e) {
                            const W t = csub(mont_mul_lazy(x[e], y[e], q, qni), q);
                            a0[c][e] = (u64)csub((W)((W)a0[c][e] + t), q);
                        }
                    }
#pragma unroll
                    for (int e = 0; e < VL; ++e) a0[c][e] = a0[c][e] * r1;
                }
            } else {
                const V o0 = *reinterpret_cast<const V*>(out + 2 * ct * Ln + rem);
                const V o1 = *reinterpret_cast<const V*>(out + (2 * ct + 1) * Ln + rem);
#pragma unroll
                for (int e = 0; e < VL; ++e) { a0[c][e] = (u64)o0[e] * r1; a1[c][e] = (u64)o1[e] * r1; }
            }
        }
        const size_t dstep = (size_t)R.L * n_d;
        auto redc = [&](u64 t) -> W { return mont_red_lazy(t, q, qni); };     // t < q 2^32 -> [0, 2q)
        if (lazy) {
            for (u32 d0 = 0; d0 < D; d0 += K) {
                const u32 dend = d0 + K < D ? d0 + K : D;
                for (u32 d = d0; d < dend; ++d) {
                    const u32 hd = hskip ? d + (d / grp + 1) * hskip : d;
                    const V h0 = *reinterpret_cast<const V*>(hint + (size_t)(2 * hd) * Ln + rem);
                    const V h1 = *reinterpret_cast<const V*>(hint + (size_t)(2 * hd + 1) * Ln + rem);
#pragma unroll
                    for (int c = 0; c < TILE; ++c) {
                        const V x = *reinterpret_cast<const V*>(dv[c] + (size_t)d * dstep);
#pragma unroll
                        for (int e = 0; e < VL; ++e) {
                            a0[c][e] += (u64)x[e] * h0[e];
                            a1[c][e] += (u64)x[e] * h1[e];
                        }
                    }
                }
                if (dend < D) {                                 // carry the running sum into the next group: t (R mod q) < 2 q^2
#pragma unroll
                    for (int c = 0; c < TILE; ++c)
#pragma unroll
                        for (int e = 0; e < VL; ++e) { a0[c][e] = (u64)redc(a0[c][e]) * r1; a1[c][e] = (u64)redc(a1[c][e]) * r1; }
                }
            }
        } else {
            // moduli too close to 2^31 for a lazy group: one reduction per product, running sum as acc = t (R mod q)
            for (u32 d = 0; d < D; ++d) {
                const u32 hd = hskip ? d + (d / grp + 1) * hskip : d;
                const V h0 = *reinterpret_cast<const V*>(hint + (size_t)(2 * hd) * Ln + rem);
                const V h1 = *reinterpret_cast<const V*>(hint + (size_t)(2 * hd + 1) * Ln + rem);
#pragma unroll
                for (int c = 0; c < TILE; ++c) {
                    const V x = *reinterpret_cast<const V*>(dv[c] + (size_t)d * dstep);
#pragma unroll
                    for (int e = 0; e < VL; ++e) {
                        a0[c][e] = (u64)csub((W)((W)a0[c][e] + csub(mont_mul_lazy(x[e], h0[e], q, qni), q)), q);
                        a1[c][e] = (u64)csub((W)((W)a1[c][e] + csub(mont_mul_lazy(x[e], h1[e], q, qni), q)), q);
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < TILE; ++c) {
            if (ct0 + c >= nct) continue;
            V r0, r1v;
#pragma unroll
            for (int e = 0; e < VL; ++e) {
                r0[e] = lazy ? csub(redc(a0[c][e]), q) : (W)a0[c][e];
                r1v[e] = lazy ? csub(redc(a1[c][e]), q) : (W)a1[c][e];
            }
            *reinterpret_cast<V*>(out + 2 * (ct0 + c) * Ln + rem) = r0;
            *reinterpret_cast<V*>(out + (2 * (ct0 + c) + 1) * Ln + rem) = r1v;
        }
    }
}

// Rescale (a,b) -> b: dst limb j-1 = q_0^-1 (src_j - reduce(lift src_0)).  q0inv_m[j] = q_0^-1 mod q_j (Montgomery).
template <typename W>
__global__ void k_rescale_drop0(DevRing<W> R, const W* src, W* dst, size_t elems, Scal<W> q0inv_m) {
    typedef typename Signed<W>::type SW;
    const size_t n = (size_t)R.n;
    const size_t L = (size_t)R.L;
    const size_t total = elems * (L - 1) * n;
    const W q0 = R.mod[0].q;
    ALCH_WALK_INIT(R.n, R.L - 1);
    ALCH_WALK(w, total, wk) {
        const size_t k = wk.k, e = wk.outer;
        const size_t j = (size_t)wk.mid + 1;
        const ModP<W> m = R.mod[j];
        const W x0 = src[(e * L) * n + k];
        const SW z = x0 > ((q0 - 1) >> 1) ? (SW)x0 - (SW)q0 : (SW)x0;
        const SW zr = reduce_signed<W>(z, m.q);
        const W d = sub_mod(src[(e * L + j) * n + k], (W)zr, m.q);
        dst[w] = mont_mul(d, q0inv_m.v[j], m);
    }
}

// Rescale b -> (a,b): dst limb 0 = 0, dst limb j+1 = q_a * src limb j.  qa_m[j+1] = q_a mod q_{j+1} (Montgomery).
template <typename W>
__global__ void k_rescale_add0(DevRing<W> Rd, const W* src, W* dst, size_t elems, Scal<W> qa_m) {
    const size_t n = (size_t)Rd.n;
    const size_t L = (size_t)Rd.L;
    const size_t total = elems * L * n;
    ALCH_WALK_INIT(Rd.n, Rd.L);
    ALCH_WALK(w, total, wk) {
        const size_t k = wk.k, j = wk.mid, e = wk.outer;
        dst[w] = j == 0 ? (W)0 : mont_mul(src[(e * (L - 1) + (j - 1)) * n + k], qa_m.v[j], Rd.mod[j]);
    }
}

// mulGCRT / divGCRT: element-wise product with a per-limb table of n words (Montgomery form).
template <typename W>
__global__ void k_mul_table(DevRing<W> R, W* data, size_t words, GTab<W> gt) {
    ALCH_WALK_INIT(R.n, R.L);
    ALCH_WALK(w, words, wk) data[w] = mont_mul(data[w], gt.p[wk.mid][wk.k], R.mod[wk.mid]);
}

// SymmSHE mulPublic (Eval.hs:132): every ring element of src times one public ring element (CRT basis, pointwise).
template <typename W>
__global__ void k_mul_bcast(DevRing<W> R, W* dst, const W* src, const W* pub, size_t words) {
    const size_t n = (size_t)R.n;
    ALCH_WALK_INIT(R.n, R.L);
    ALCH_WALK(w, words, wk) {
        const ModP<W> m = R.mod[wk.mid];
        dst[w] = mont_mul(mont_mul(src[w], m.r2, m), pub[(size_t)wk.mid * n + wk.k], m);
    }
}

// SymmSHE addPublic (Eval.hs:131): one public ring element added to the c0 of every ciphertext (elements 0, 2, 4, ..).
template <typename W>
__global__ void k_add_bcast(DevRing<W> R, W* dst, const W* pub, size_t cts) {
    const size_t n = (size_t)R.n, Ln = (size_t)R.L * n;
    ALCH_WALK_INIT(R.n, R.L);
    ALCH_WALK(w, cts * Ln, wk) {
        const size_t ct = wk.outer, rem = (size_t)wk.mid * n + wk.k;
        W* p = dst + 2 * ct * Ln + rem;
        *p = add_mod(*p, pub[rem], R.mod[wk.mid].q);
    }
}

// SymmSHE addPublic in one pass: dst = src * s_j, c0 components (even elements) += pub.  Element-major walk with VW-word pieces.
template <typename W, int VW = 1>
__global__ void k_scale_add_bcast(DevRing<W> R, W* dst, const W* src, const W* pub, size_t words, Scal<W> sm) {
    typedef Pack<W, VW> P;
    ALCH_WALK_INIT(R.n / VW, R.L);
    ALCH_WALK(w, words / VW, wk) {
        P x = reinterpret_cast<const P*>(src)[w];
        const ModP<W> mp = R.mod[wk.mid];
#pragma unroll
        for (int c = 0; c < VW; ++c) x.v[c] = mont_mul(x.v[c], sm.v[wk.mid], mp);
        if ((wk.outer & 1u) == 0) {
            const P b = reinterpret_cast<const P*>(pub)[(size_t)wk.mid * (R.n / VW) + wk.k];
#pragma unroll
            for (int c = 0; c < VW; ++c) x.v[c] = add_mod(x.v[c], b.v[c], mp.q);
        }
        reinterpret_cast<P*>(dst)[w] = x;
    }
}

// Tunnel, step 1: the E'-coefficients of (c0, c1) embedded into S' (coeffs + embedPow as one index gather; toMSD's
// per-limb scalar folded in).  in: [ct][2][L - dup][n_r] -- the ciphertexts may live `dup` limbs below the tunnel's ring
// (PT2CT's modSwitch_ in front of tunnel_, PT2CT.hs:224-229: x -> (0, q_a x), the factor folded into s_m by the host);
// x0 / x1: [ct][d_rel][Lx][n_s] holding the limbs xoff .. xoff + Lx - 1 (compact: the zero limbs are left out).
template <typename W, int VW = 1>
__global__ void k_tunnel_gather(DevRing<W> Rs, const W* in0, const W* in1, W* x0, W* x1, const int32_t* table, u32 d_rel, u32 n_r, size_t nct,
                                Scal<W> s_m, int scale, u32 Lx, u32 xoff, u32 dup) {
    // in0 / in1: where the c0 / c1 components are read from (same [ct][2][..] layout: c0 may come from a scratch copy that went
    // through lInv while c1 is read in place)
    typedef Pack<W, VW> P;
    typedef Pack<int32_t, VW> PI;
    const size_t n = (size_t)Rs.n, Lin = (size_t)Rs.L - dup;
    const size_t per_ct = (size_t)d_rel * Lx * n;
    // words as [ct * 2 + comp][i * Lx + limb'][k]; a thread gathers VW consecutive k and stores them as one piece
    ALCH_WALK_INIT(Rs.n / VW, d_rel * Lx);
    ALCH_WALK(w, nct * 2 * per_ct / VW, wk) {
        const size_t ct = wk.outer >> 1, comp = wk.outer & 1, k = (size_t)wk.k * VW;
        const u32 i = wk.mid / Lx, limb = wk.mid - i * Lx + xoff;
        const size_t r2 = (size_t)wk.mid * n + k;
        const PI src = *reinterpret_cast<const PI*>(table + i * n + k);
        P v;
#pragma unroll
        for (int c = 0; c < VW; ++c) {
            W x = 0;
            if (src.v[c] >= 0 && limb >= dup) {
                x = (comp ? in1 : in0)[((2 * ct + comp) * Lin + (limb - dup)) * (size_t)n_r + (size_t)src.v[c]];
                if (scale) x = mont_mul(x, s_m.v[limb], Rs.mod[limb]);
            }
            v.v[c] = x;
        }
        *reinterpret_cast<P*>((comp ? x1 : x0) + ct * per_ct + r2) = v;
    }
}

// Tunnel, step 2: c0' = sum_i crt(x0_i) * y_i (evalLin on the constant term), c1' = 0.  out: [ct][2][L][n];
// x0crt: [ct][d_rel][Lx][n] holding the limbs xoff .. (the limbs in front of xoff are zero).
template <typename W, int VW = 1>
__global__ void k_tunnel_lin(DevRing<W> Rs, W* out, const W* x0crt, const W* lin, u32 d_rel, size_t nct, u32 Lx, u32 xoff,
                             const u32* slot_e, u32 n_x) {
    // slot_e != null: x0crt holds CRT vectors of dimension n_x over E' ([ct][d_rel][Lx][n_x]); slot s of S' reads entry slot_e[s]
    typedef Pack<W, VW> P;
    const size_t n = (size_t)Rs.n, Ln = (size_t)Rs.L * n, Lxn = (size_t)Lx * (slot_e ? (size_t)n_x : n);
    ALCH_WALK_INIT(Rs.n / VW, Rs.L);
    ALCH_WALK(w, nct * Ln / VW, wk) {
        const size_t ct = wk.outer, rem = (size_t)wk.mid * n + (size_t)wk.k * VW;
        const ModP<W> m = Rs.mod[wk.mid];
        P acc, zero;
#pragma unroll
        for (int c = 0; c < VW; ++c) { acc.v[c] = 0; zero.v[c] = 0; }
        if (wk.mid >= xoff) {
            const size_t xr = slot_e ? (size_t)(wk.mid - xoff) * n_x : (size_t)(wk.mid - xoff) * n + (size_t)wk.k * VW;
            for (u32 i = 0; i < d_rel; ++i) {
                P x;
                if (slot_e) {
#pragma unroll
                    for (int c = 0; c < VW; ++c) x.v[c] = x0crt[(ct * d_rel + i) * Lxn + xr + slot_e[(size_t)wk.k * VW + c]];
                } else {
                    x = *reinterpret_cast<const P*>(x0crt + (ct * d_rel + i) * Lxn + xr);
                }
                const P y = *reinterpret_cast<const P*>(lin + (size_t)i * Ln + rem);
#pragma unroll
                for (int c = 0; c < VW; ++c) acc.v[c] = add_mod(acc.v[c], mont_mul(x.v[c], y.v[c], m), m.q);
            }
        }
        *reinterpret_cast<P*>(out + 2 * ct * Ln + rem) = acc;
        *reinterpret_cast<P*>(out + (2 * ct + 1) * Ln + rem) = zero;
    }
}

// ---- tunnels between two-power rings of the radix-16 engine (do_tunnel_pow2) ---------------------------------------------------
// Both rings are Z_q[X]/(X^n + 1); with d = d_rel = max(1, n_r / n_s) and n_d = n_r / d (the dimension the transforms run at):
//   coeffs     E'-coefficient i of a Pow vector over R' is its stride-d subsequence starting at i (zeta_e = X^d; g = 1, l = identity)
//   embedCRT   crt_S'(embedPow x)[k] = crt_R'(x)[k >> sh], n_s = 2^sh n_d: the slot rule is bit-reversed, so the 2^sh slots of S'
//              above a slot of the smaller ring are consecutive (sh = 0 in the down direction, where E' = S')
// Step 1, the gather: from the Pow copy of (c0, c1) over R' ([ct][2][Lin][n_r], Lin = L - dup limbs: the ciphertexts may sit dup limbs
// below the tunnel's ring, the added moduli are folded into s_m) to
//   x0   [ct][d][Lin][n_d]        the E'-coefficients of c0 times s_m (null: not wanted -- CRT input in the up direction)
//   dst1 TRIV:  [ct][d][Lin][L][n_d]  the TrivGad digits of the coefficients of c1 s_m: centred lift of limb i reduced into every limb
//        !TRIV: [ct][d][L][n_d]       the coefficients of c1 s_m themselves, zero in the dup leading limbs (BaseBGad 2 decomposes later)
// A thread owns VL consecutive positions of G = min(d, VL) neighbouring coefficients: its VL x G source words are G (d < VL) or VL
// whole 16-byte pieces, transposed in registers, so every access is a 16-byte one.
template <typename W, int G, bool TRIV>
__global__ void __launch_bounds__(256) k_tun2_gather(DevRing<W> Rs, const W* in, W* x0, W* dst1, u32 d, u32 n_d, size_t nct, Scal<W> s_m, int scale,
                                                     u32 dup, int balanced) {
    typedef typename Vec4<W>::type V;
    typedef typename Signed<W>::type SW;
    constexpr int VL = Vec4<W>::LANES;
    const u32 L = (u32)Rs.L, Lin = L - dup;
    const u32 Lw = TRIV ? Lin : L;                               // limbs walked per component
    const u32 c0 = x0 ? 0u : 1u, ncomp = 2u - c0;
    const u32 nv = n_d / VL, ng = d / G;
    const size_t n_r = (size_t)n_d * d;
    ALCH_WALK_INIT(nv * ng, ncomp * Lw);
    ALCH_WALK(w, nct * ncomp * Lw * ng * nv, wk) {
        const size_t ct = wk.outer;
        const u32 comp = wk.mid / Lw + c0, limb = wk.mid % Lw + (TRIV ? dup : 0u);
        const u32 k4 = (wk.k % nv) * VL, i0 = (wk.k / nv) * G;
        V t[G];                                                  // t[a][kk]: coefficient i0 + a, position k4 + kk
        if (limb < dup) {
#pragma unroll
            for (int a = 0; a < G; ++a)
#pragma unroll
                for (int e = 0; e < VL; ++e) t[a][e] = 0;
        } else {
            const W* src = in + ((2 * ct + comp) * Lin + (limb - dup)) * n_r;
            const ModP<W> m = Rs.mod[limb];
            if constexpr (G == VL) {                             // d >= VL: one piece per position, VL coefficients wide
#pragma unroll
                for (int c = 0; c < VL; ++c) {
                    const V p = *reinterpret_cast<const V*>(src + (size_t)(k4 + c) * d + i0);
#pragma unroll
                    for (int a = 0; a < G; ++a) t[a][c] = p[a];
                }
            } else {                                             // d = G < VL: the VL positions of all d coefficients are d consecutive pieces
#pragma unroll
                for (int c = 0; c < G; ++c) {
                    const V p = *reinterpret_cast<const V*>(src + (size_t)k4 * G + c * VL);
#pragma unroll
                    for (int e = 0; e < VL; ++e) t[(c * VL + e) % G][(c * VL + e) / G] = p[e];
                }
            }
            if (scale) {
#pragma unroll
                for (int a = 0; a < G; ++a)
#pragma unroll
                    for (int e = 0; e < VL; ++e) t[a][e] = mont_mul(t[a][e], s_m.v[limb], m);
            }
        }
#pragma unroll
        for (int a = 0; a < G; ++a) {
            const size_t ci = ct * d + i0 + a;
            if (comp == 0) {                                     // compact: the dup leading limbs (walked for !TRIV only) have no place in x0
                if (limb >= dup) *reinterpret_cast<V*>(x0 + (ci * Lin + (limb - dup)) * (size_t)n_d + k4) = t[a];
            } else if (!TRIV) {
                *reinterpret_cast<V*>(dst1 + (ci * L + limb) * (size_t)n_d + k4) = t[a];
            } else {
                const W qi = Rs.mod[limb].q, hq = (qi - 1) >> 1;
                for (u32 j = 0; j < L; ++j) {
                    const W qj = Rs.mod[j].q;
                    V r;
#pragma unroll
                    for (int e = 0; e < VL; ++e) {
                        const SW z = t[a][e] > hq ? (SW)t[a][e] - (SW)qi : (SW)t[a][e];
                        r[e] = balanced ? (W)(z < 0 ? z + (SW)qj : z) : (W)reduce_signed<W>(z, qj);
                    }
                    *reinterpret_cast<V*>(dst1 + ((ci * Lin + (limb - dup)) * L + j) * (size_t)n_d + k4) = r;
                }
            }
        }
    }
}

// Step 2, the hint inner product with slot replication: for S' slot k and TILE ciphertexts sharing every hint piece,
//   c0'[k] = sum_i x0crt_i[k >> sh] lin_i[k] + sum_d digit_d[k >> sh] hint_{d,0}[k],   c1'[k] = sum_d digit_d[k >> sh] hint_{d,1}[k]
// (evalLin's constant term is the starting value, as in k_tunnel_mac_e).  A thread owns one 16-byte piece of S' slots; the VL digit
// words behind it lie in ONE aligned 16-byte piece of the small vector (all VL the same word once sh >= log2 VL), which it loads whole and
// picks from -- the lanes of a wavefront that share a piece are served by one request, so a digit word is fetched once per wavefront
// pass, not once per replicated slot, and every access stays a 16-byte one.
// digits: [ct][D][L][n_d], digit d uses hint row hd = d + (d / grp + 1) hskip (compact TrivGad digits of ciphertexts hskip limbs below the
// ring; hskip = 0: hd = d).  x0: element (ct, i) limb j >= xoff at x0 + ct x0_cts + (i Lx + j - xoff) n_d; x0_scale: times s_m on the fly
// (CRT input in the up direction, where c0 is read in place).  32-bit words: lazy 64-bit groups of K = floor((2^32 - 1) / q) - 2 products
// per reduction, product-at-a-time where K < 2, exactly as k_tunnel_mac_e; 64-bit words: one Montgomery product at a time.
template <typename W> __device__ __forceinline__ W tun2_pick(typename Vec4<W>::type p, u32 i);
template <> __device__ __forceinline__ u32 tun2_pick<u32>(Vec4<u32>::type p, u32 i) { const u32 lo = (i & 1) ? p[1] : p[0], hi = (i & 1) ? p[3] : p[2]; return (i & 2) ? hi : lo; }
template <> __device__ __forceinline__ u64 tun2_pick<u64>(Vec4<u64>::type p, u32 i) { return (i & 1) ? p[1] : p[0]; }

template <typename W, int TILE>
__global__ void __launch_bounds__(256) k_tun2_mac(DevRing<W> R, W* out, const W* digits, const W* hint, size_t nct, u32 D, u32 grp, u32 hskip, u32 sh,
                                                  u32 n_d, const W* x0, size_t x0_cts, const W* lin, u32 d_rel, u32 Lx, u32 xoff, Scal<W> s_m,
                                                  int x0_scale) {
    typedef typename Vec4<W>::type V;
    constexpr int VL = Vec4<W>::LANES;
    const size_t n = (size_t)R.n;
    const size_t Ln = (size_t)R.L * n;
    const size_t ntile = (nct + TILE - 1) / TILE;
    const size_t nv = n / VL;
    ALCH_WALK_INIT(nv, R.L);
    ALCH_WALK(w, ntile * (size_t)R.L * nv, wk) {
        const size_t ct0 = wk.outer * TILE, rem = (size_t)wk.mid * n + (size_t)wk.k * VL;
        const u32 limb = wk.mid;
        const ModP<W> m = R.mod[limb];
        const W q = m.q, qni = m.qni;
        // the digit words behind this piece: word (k + e) >> sh, all inside the aligned piece that starts at `se`
        const u32 k0 = wk.k * (u32)VL;
        const u32 se = (k0 >> sh) & ~(u32)(VL - 1);
        u32 pick[VL];
#pragma unroll
        for (int e = 0; e < VL; ++e) pick[e] = ((k0 + (u32)e) >> sh) - se;
        auto spread = [&](V p) -> V {
            if (sh == 0) return p;
            V x;
#pragma unroll
            for (int e = 0; e < VL; ++e) x[e] = tun2_pick<W>(p, pick[e]);
            return x;
        };
        bool lazy = false;
        u32 K = 0;
        if constexpr (sizeof(W) == 4) {
            K = lazy_group((u32)q);                                // (K + 2) q < 2^32
            lazy = K >= 2;
        }
        const u64 r1 = lazy ? (u64)m.r1 : 1;                       // not lazy: the accumulators hold the running sum itself, in [0, q)
        u64 a0[TILE][VL], a1[TILE][VL];
        const W* dv[TILE];
#pragma unroll
        for (int c = 0; c < TILE; ++c) {
            const size_t ct = ct0 + c < nct ? ct0 + c : ct0;       // a dead lane of the tile recomputes ciphertext ct0 and stores nothing
            dv[c] = digits + (ct * (size_t)D * R.L + limb) * (size_t)n_d + se;
#pragma unroll
            for (int e = 0; e < VL; ++e) { a0[c][e] = 0; a1[c][e] = 0; }
            if (limb >= xoff) {
                for (u32 i = 0; i < d_rel; ++i) {
                    const V x = spread(*reinterpret_cast<const V*>(x0 + ct * x0_cts + ((size_t)i * Lx + (limb - xoff)) * (size_t)n_d + se));
                    const V y = *reinterpret_cast<const V*>(lin + (size_t)i * Ln + rem);
#pragma unroll
                    for (int e = 0; e < VL; ++e) {
                        const W xs = x0_scale ? mont_mul(x[e], s_m.v[limb], m) : x[e];
                        a0[c][e] = (u64)add_mod((W)a0[c][e], mont_mul(xs, y[e], m), q);
                    }
                }
#pragma unroll
                for (int e = 0; e < VL; ++e) a0[c][e] = a0[c][e] * r1;
            }
        }
        const size_t dstep = (size_t)R.L * n_d;
        if (lazy) {
            if constexpr (sizeof(W) == 4) {
                auto redc = [&](u64 t) -> u32 { return mont_red_lazy(t, (u32)q, (u32)qni); };     // t < q 2^32 -> [0, 2q)
                for (u32 d0 = 0; d0 < D; d0 += K) {
                    const u32 dend = d0 + K < D ? d0 + K : D;
                    for (u32 d = d0; d < dend; ++d) {
                        const u32 hd = hskip ? d + (d / grp + 1) * hskip : d;
                        const V h0 = *reinterpret_cast<const V*>(hint + (size_t)(2 * hd) * Ln + rem);
                        const V h1 = *reinterpret_cast<const V*>(hint + (size_t)(2 * hd + 1) * Ln + rem);
#pragma unroll
                        for (int c = 0; c < TILE; ++c) {
                            const V x = spread(*reinterpret_cast<const V*>(dv[c] + (size_t)d * dstep));
#pragma unroll
                            for (int e = 0; e < VL; ++e) {
                                a0[c][e] += (u64)x[e] * h0[e];
                                a1[c][e] += (u64)x[e] * h1[e];
                            }
                        }
                    }
                    if (dend < D) {                                 // carry the running sum into the next group: t (R mod q) < 2 q^2
#pragma unroll
                        for (int c = 0; c < TILE; ++c)
#pragma unroll
                            for (int e = 0; e < VL; ++e) { a0[c][e] = (u64)redc(a0[c][e]) * r1; a1[c][e] = (u64)redc(a1[c][e]) * r1; }
                    }
                }
#pragma unroll
                for (int c = 0; c < TILE; ++c)
#pragma unroll
                    for (int e = 0; e < VL; ++e) { a0[c][e] = csub(redc(a0[c][e]), q); a1[c][e] = csub(redc(a1[c][e]), q); }
            }
        } else {
            for (u32 d = 0; d < D; ++d) {
                const u32 hd = hskip ? d + (d / grp + 1) * hskip : d;
                const V h0 = *reinterpret_cast<const V*>(hint + (size_t)(2 * hd) * Ln + rem);
                const V h1 = *reinterpret_cast<const V*>(hint + (size_t)(2 * hd + 1) * Ln + rem);
#pragma unroll
                for (int c = 0; c < TILE; ++c) {
                    const V x = spread(*reinterpret_cast<const V*>(dv[c] + (size_t)d * dstep));
#pragma unroll
                    for (int e = 0; e < VL; ++e) {
                        a0[c][e] = (u64)add_mod((W)a0[c][e], mont_mul(x[e], h0[e], m), q);
                        a1[c][e] = (u64)add_mod((W)a1[c][e], mont_mul(x[e], h1[e], m), q);
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < TILE; ++c) {
            if (ct0 + c >= nct) continue;
            V r0, r1v;
#pragma unroll
            for (int e = 0; e < VL; ++e) { r0[e] = (W)a0[c][e]; r1v[e] = (W)a1[c][e]; }
            *reinterpret_cast<V*>(out + 2 * (ct0 + c) * Ln + rem) = r0;
            *reinterpret_cast<V*>(out + (2 * (ct0 + c) + 1) * Ln + rem) = r1v;
        }
    }
}

// Rescale b -> (a_1, .., a_dup, b): dst limb j < dup = 0, dst limb j >= dup = (prod of the added moduli) * src limb j - dup.
template <typename W>
__global__ void k_rescale_up(DevRing<W> Rd, const W* src, W* dst, size_t elems, int dup, Scal<W> mult_m) {
    const size_t n = (size_t)Rd.n, L = (size_t)Rd.L, Ls = L - (size_t)dup;
    ALCH_WALK_INIT(Rd.n, Rd.L);
    ALCH_WALK(w, elems * L * n, wk) {
        const size_t k = wk.k, j = wk.mid, e = wk.outer;
        dst[w] = j < (size_t)dup ? (W)0 : mont_mul(src[(e * Ls + (j - dup)) * n + k], mult_m.v[j], Rd.mod[j]);
    }
}

template <typename W>
__global__ void k_checksum(const W* data, size_t words, u64* sum, u64 w0) {
    u64 acc = 0;
    for (size_t w = blockIdx.x * (size_t)blockDim.x + threadIdx.x; w < words; w += (size_t)gridDim.x * blockDim.x)
        acc += splitmix64(((u64)w + w0) ^ ((u64)data[w] << 20));
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd((unsigned long long*)sum, (unsigned long long)acc);
}

#include "kernel_lift.hpp"
#include "kernel_plain.hpp"
#include "kernel_rlwe.hpp"
#include "kernel_automorph.hpp"
#include "kernel_hoist.hpp"
#include "kernel_lincomb.hpp"

static inline unsigned ew_grid(size_t items) {
    size_t g = (items + 255) / 256;
    if (g > 2048) g = 2048;
    if (g < 1) g = 1;
    return (unsigned)g;
}

// ------------------------------------------------------------------------------------------------------
// ring construction
// ------------------------------------------------------------------------------------------------------
template <typename W>
static int build_dev_ring(alch_ring* r, DevRing<W>& d) {
    const size_t n = r->n;
    const int L = r->L;
    std::vector<W> all(2 * (size_t)L * n);
    HIP_TRY(hipMalloc(&r->tables, all.size() * sizeof(W)));
    memset(&d, 0, sizeof d);
    d.L = L;
    d.logn = r->logn;
    d.n = r->n;
    u64 maxhalf = 0;
    for (int j = 0; j < L; ++j) maxhalf = std::max(maxhalf, (r->q[j] - 1) / 2);
    for (int j = 0; j < L; ++j) {
        const u64 q = r->q[j];
        d.mod[j] = make_modp<W>(q);
        const u64 psi = h_root(q, r->m);
        std::vector<W> f, inv;
        h_build_twiddles<W>(q, psi, r->logn, f, inv);
        memcpy(&all[(size_t)(2 * j) * n], f.data(), n * sizeof(W));
        memcpy(&all[(size_t)(2 * j + 1) * n], inv.data(), n * sizeof(W));
        d.twf[j] = reinterpret_cast<W*>(r->tables) + (size_t)(2 * j) * n;
        d.twi[j] = reinterpret_cast<W*>(r->tables) + (size_t)(2 * j + 1) * n;
        const u64 ninv = h_powmod(n % q, q - 2, q);
        const u64 r1 = d.mod[j].r1;
        d.ninv_m[j] = (W)h_mulmod(ninv, r1, q);
        // inv[1] is tw^-1[1] * R; times n^-1 stays in Montgomery form
        d.w1ninv_m[j] = (W)h_mulmod((u64)inv[1], ninv, q);
        d.dig_off[j] = (W)(((maxhalf + q - 1) / q) * q);
    }
    HIP_TRY(hipMemcpy(r->tables, all.data(), all.size() * sizeof(W), hipMemcpyHostToDevice));
    if (sizeof(W) == 4) {
        // forward and inverse twiddles once more as Plantard constants: tw[k] = psi^brev(k), twi[k] = psi^-brev(k) (plain residues)
        std::vector<u64> pl(2 * (size_t)L * n);
        for (int j = 0; j < L; ++j) {
            const u64 q = r->q[j];
            const u64 psi = h_root(q, r->m), ipsi = h_powmod(psi, q - 2, q);
            std::vector<u64> pw(n), ipw(n);
            u64 acc = 1, iacc = 1;
            for (size_t i = 0; i < n; ++i) { pw[i] = acc; ipw[i] = iacc; acc = h_mulmod(acc, psi, q); iacc = h_mulmod(iacc, ipsi, q); }
            for (size_t k = 0; k < n; ++k) {
                const u32 e = h_brev((u32)k, r->logn);
                pl[(size_t)(2 * j) * n + k] = h_plant_const(pw[e], q);
                pl[(size_t)(2 * j + 1) * n + k] = h_plant_const(ipw[e], q);
            }
        }
        HIP_TRY(hipMalloc(&r->tables_p, pl.size() * sizeof(u64)));
        HIP_TRY(hipMemcpy(r->tables_p, pl.data(), pl.size() * sizeof(u64), hipMemcpyHostToDevice));
        for (int j = 0; j < L; ++j) {
            d.twp[j] = reinterpret_cast<const u64*>(r->tables_p) + (size_t)(2 * j) * n;
            d.twpi[j] = reinterpret_cast<const u64*>(r->tables_p) + (size_t)(2 * j + 1) * n;
        }
    } else {
        // 64-bit rings: the transforms multiply by Shoup pairs (plain twiddle, floor(w 2^64 / q)); the Montgomery
        // tables above still serve the hand-written stage 0 of the split kernels
        std::vector<Sh64> sh(2 * (size_t)L * n);
        for (int j = 0; j < L; ++j) {
            const u64 q = r->q[j];
            const u64 psi = h_root(q, r->m), ipsi = h_powmod(psi, q - 2, q);
            std::vector<u64> pw(n), ipw(n);
            u64 a = 1, b = 1;
            for (size_t i = 0; i < n; ++i) { pw[i] = a; ipw[i] = b; a = h_mulmod(a, psi, q); b = h_mulmod(b, ipsi, q); }
            for (size_t k = 0; k < n; ++k) {
                const u32 e = h_brev((u32)k, r->logn);
                sh[(size_t)(2 * j) * n + k] = h_shoup_const(pw[e], q);
                sh[(size_t)(2 * j + 1) * n + k] = h_shoup_const(ipw[e], q);
            }
        }
        HIP_TRY(hipMalloc(&r->tables_p, sh.size() * sizeof(Sh64)));
        HIP_TRY(hipMemcpy(r->tables_p, sh.data(), sh.size() * sizeof(Sh64), hipMemcpyHostToDevice));
        for (int j = 0; j < L; ++j) {
            d.tws[j] = reinterpret_cast<const Sh64*>(r->tables_p) + (size_t)(2 * j) * n;
            d.twsi[j] = reinterpret_cast<const Sh64*>(r->tables_p) + (size_t)(2 * j + 1) * n;
        }
    }
    return ALCH_OK;
}

template <typename W> static GenDev<W>& gen_dev(alch_ring* r);
template <> GenDev<u32>& gen_dev<u32>(alch_ring* r) { return r->g32; }
template <> GenDev<u64>& gen_dev<u64>(alch_ring* r) { return r->g64; }

// General-index ring: moduli / Montgomery constants into DevRing, pass plan and tables into GenDev.
template <typename W>
static int build_gen_ring(alch_ring* r, DevRing<W>& d, GenDev<W>& g) {
    const GenHost& h = r->gh;
    const int L = r->L;
    memset(&d, 0, sizeof d);
    memset(&g, 0, sizeof g);
    d.L = L; d.logn = 0; d.n = h.n;
    g.n = h.n; g.npass = h.npass; g.nfact = h.nfact; g.rad = h.rad;
    for (int i = 0; i < h.npass; ++i) g.pass[i] = h.pass[i];
    for (int i = 0; i < h.nfact; ++i) g.fact[i] = h.fact[i];
    g.plain = (!r->has_crt && !r->zdom) ? 1 : 0;
    g.smallq = (r->has_crt && sizeof(W) == 4) ? 2 : 0;                            // the least level over the limbs (dense_level)
    for (int j = 0; j < L && g.smallq; ++j) g.smallq = std::min(g.smallq, dense_level(r->q[j]));
    u64 maxhalf = 0;
    for (int j = 0; j < L; ++j) maxhalf = std::max(maxhalf, r->q[j] ? (r->q[j] - 1) / 2 : 0);
    if (!r->has_crt) {
        for (int j = 0; j < L; ++j) {
            d.mod[j].q = (W)r->q[j]; d.mod[j].qni = 0; d.mod[j].r1 = 1; d.mod[j].r2 = 1;
            // plain inverse of the odd radical (0 when it is not a unit); the integers divide exactly instead
            u64 inv = 0;
            if (r->q[j]) {
                // extended Euclid
                int64_t r0 = (int64_t)r->q[j], r1 = (int64_t)(h.rad % r->q[j]), t0 = 0, t1 = 1;
                while (r1) { int64_t k = r0 / r1, r2 = r0 - k * r1, t2 = t0 - k * t1; r0 = r1; r1 = r2; t0 = t1; t1 = t2; }
                inv = r0 == 1 ? (u64)(((t0 % (int64_t)r->q[j]) + (int64_t)r->q[j]) % (int64_t)r->q[j]) : 0;
            }
            g.radinv_m[j] = (W)inv;
        }
        return ALCH_OK;
    }
    const size_t per_limb = 2 * (size_t)h.block_words + 2 * (size_t)h.n;
    std::vector<W> all(per_limb * L);
    HIP_TRY(hipMalloc(&r->gen_tables, all.size() * sizeof(W)));
    const int bits = 8 * (int)sizeof(W);
    for (int j = 0; j < L; ++j) {
        const u64 q = r->q[j];
        d.mod[j] = make_modp<W>(q);
        d.dig_off[j] = (W)(((maxhalf + q - 1) / q) * q);
        const u64 r1 = h_powmod(2, (u64)bits, q);
        std::vector<u64> f, iv, gc, gci;
        u64 iscale = 1;
        if (!gen_tables(h, q, f, iv, gc, gci, iscale)) return fail(ALCH_E_INVALID, "general-index table construction failed");
        W* base = all.data() + per_limb * j;
        for (u32 k = 0; k < h.block_words; ++k) { base[k] = (W)h_mulmod(f[k], r1, q); base[h.block_words + k] = (W)h_mulmod(iv[k], r1, q); }
        for (u32 k = 0; k < h.n; ++k) { base[2 * h.block_words + k] = (W)h_mulmod(gc[k], r1, q); base[2 * h.block_words + h.n + k] = (W)h_mulmod(gci[k], r1, q); }
        W* dev = reinterpret_cast<W*>(r->gen_tables) + per_limb * j;
        g.tabf[j] = dev; g.tabi[j] = dev + h.block_words;
        g.gcrt[j] = dev + 2 * h.block_words; g.gcrt_inv[j] = dev + 2 * h.block_words + h.n;
        g.iscale_m[j] = (W)h_mulmod(iscale, r1, q);
        g.radinv_m[j] = (h.rad % q) ? (W)h_mulmod(h_invmod(h.rad % q, q), r1, q) : (W)0;
    }
    HIP_TRY(hipMemcpy(r->gen_tables, all.data(), all.size() * sizeof(W), hipMemcpyHostToDevice));
    return ALCH_OK;
}

static bool two_power_engine(uint32_t m) { return m >= 32 && (m & (m - 1)) == 0; }

// Status order of alch_ring_create (the order a Lol host needs, haskell/.../GT.hs `ringFor`):
//   1. malformed arguments                                  -> ALCH_E_INVALID
//   2. NO CRT BASIS over the base ring -- a modulus that is composite, 2, or a prime that is not 1 mod m: the cases in which Lol's
//      `crtFuncs` / `crtInfo` answer Nothing for ZqBasic (CRTrans Maybe needs a prime q with m | q - 1; pairs need both) -> ALCH_E_NO_CRT,
//      whatever the index: it is a property of (m, q), not of this backend; the caller falls back to alch_ring_create_nocrt
//   3. a CRT basis exists but this backend does not serve the ring (prime factor of m above 13, a limb-polynomial larger than the
//      LDS, q >= 2^62)                                      -> ALCH_E_UNSUPPORTED: the caller keeps that (m, r) on lol-cpp as a whole
// ALCH_E_NOT_PRIME is only returned by alch_host_root.
static int classify_crt_moduli(uint32_t m, int L, const uint64_t* q) {
    if (!q || L < 1 || L > MAXL) return fail(ALCH_E_INVALID, "alch_ring_create: need 1 <= L <= 8 moduli");
    if (m < 1) return fail(ALCH_E_INVALID, "cyclotomic index must be >= 1");
    for (int j = 0; j < L; ++j) {
        if (q[j] < 2) return fail(ALCH_E_INVALID, "alch_ring_create: moduli must be >= 2 (the integers: alch_ring_create_nocrt with q = 0)");
        for (int i = 0; i < j; ++i)
            if (q[i] == q[j]) return fail(ALCH_E_INVALID, "RNS moduli must be distinct");
    }
    for (int j = 0; j < L; ++j) {
        if (q[j] >= (1ull << 62)) continue;                     // classified below as unsupported (primality is not tested up there)
        if (q[j] < 3 || !h_is_prime(q[j]))
            return fail(ALCH_E_NO_CRT, "modulus " + std::to_string(q[j]) + " is not an odd prime: no CRT basis over Z_q (Lol: crtFuncs = Nothing)");
        if ((q[j] - 1) % m) return fail(ALCH_E_NO_CRT, "modulus " + std::to_string(q[j]) + " is not 1 mod m: no CRT basis (Lol: crtFuncs = Nothing)");
    }
    for (int j = 0; j < L; ++j)
        if (q[j] >= (1ull << 62)) return fail(ALCH_E_UNSUPPORTED, "modulus must be below 2^62");
    return ALCH_OK;
}

// Argument checks of a general-index ring (or of a ring without CRT basis).  Fills gh; word size out.
static int validate_gen_args(uint32_t m, int L, const uint64_t* q, bool nocrt, GenHost& gh, int* word_out, bool* zdom_out) {
    if (!q || L < 1 || L > MAXL) return fail(ALCH_E_INVALID, "alch_ring_create: need 1 <= L <= 8 moduli");
    if (m < 1) return fail(ALCH_E_INVALID, "cyclotomic index must be >= 1");
    if (!nocrt) { const int rc = classify_crt_moduli(m, L, q); if (rc != ALCH_OK) return rc; }
    if (!gen_plan(m, gh)) return fail(ALCH_E_UNSUPPORTED, "cyclotomic index " + std::to_string(m) + ": " + gh.error);
    bool all32 = true, zdom = false;
    for (int j = 0; j < L; ++j) {
        if (nocrt) {
            if (q[j] == 0) { zdom = true; continue; }
            if (q[j] < 2 || q[j] >= (1ull << 31)) return fail(ALCH_E_UNSUPPORTED, "a ring without CRT basis takes moduli 2 <= q < 2^31, or 0 for the integers");
            continue;
        }
        if (q[j] >= (1ull << 31)) all32 = false;
    }
    if (zdom) for (int j = 0; j < L; ++j) if (q[j] != 0) return fail(ALCH_E_INVALID, "modulus 0 (the integers) cannot be mixed with other moduli");
    const int word = (zdom || !all32) ? 8 : 4;
    if ((size_t)gh.n * (size_t)word > 163840) return fail(ALCH_E_UNSUPPORTED, "ring dimension too large: a limb-polynomial must fit the 160 KiB LDS");
    *word_out = word;
    *zdom_out = zdom;
    return ALCH_OK;
}

static int validate_ring_args(uint32_t m, int L, const uint64_t* q, int* logn_out, int* word_out) {
    if (!two_power_engine(m)) return fail(ALCH_E_UNSUPPORTED, "internal: not a two-power index >= 32");
    const int rc = classify_crt_moduli(m, L, q);
    if (rc != ALCH_OK) return rc;
    int logn = 0;
    while ((1u << logn) < m / 2) ++logn;
    bool all32 = true;
    for (int j = 0; j < L; ++j) if (q[j] >= (1ull << 31)) all32 = false;
    const int word = all32 ? 4 : 8;
    const int maxlog = all32 ? 16 : 15;        // the top size of each word runs as two LDS-resident halves
    if (logn > maxlog) return fail(ALCH_E_UNSUPPORTED, "ring dimension too large (n <= 2^16 for 32-bit, 2^15 for 64-bit residues)");
    *logn_out = logn;
    *word_out = word;
    return ALCH_OK;
}

// ------------------------------------------------------------------------------------------------------
// limb-count selection (host only): PT2CT's type-level modulus arithmetic, restated
// ------------------------------------------------------------------------------------------------------
// Crypto/Alchemy/Interpreter/PT2CT/Noise.hs:107-170 (units of a modulus, shortest prefix with enough units) and
// Crypto/Alchemy/Interpreter/PT2CT.hs:132-140 (KSPNoise), :160-177 (mul_), :207-229 (linearCyc_), :234-249
// (CTPNoise2Units, KSPNoise2Units, Units2CTPNoise), :281-296 (the constants).
extern "C" int alch_modulus_units(uint64_t q) try {
    if (q < 2) return 0;
    return (int)std::floor(std::log2((double)q) / 6.1);          // mkModulus: floor (logBase 2 q / pNoiseUnit)
} catch (...) { return abi_catch(); }

extern "C" int alch_select_limbs(const uint64_t* moduli, int n_moduli, int op, int gadget, int p_noise_out, int* L_in,
                                 int* L_hint, int* L_out, int* p_noise_in) try {
    if (!moduli || n_moduli < 1 || p_noise_out < 0) return fail(ALCH_E_INVALID, "alch_select_limbs: bad argument");
    if (op != ALCH_OP_MUL && op != ALCH_OP_TUNNEL) return fail(ALCH_E_INVALID, "alch_select_limbs: unknown op");
    const int gw = hintgad::gadget_width(gadget);
    if (gw < 0) return fail(ALCH_E_INVALID, "alch_select_limbs: unknown gadget");
    const int MinUnits = (int)std::ceil(12 / 6.1), MulPNoise = (int)std::ceil(18 / 6.1), KSAccumPNoise = (int)std::ceil(12 / 6.1),
              Max32BitUnits = (int)std::ceil(30.5 / 6.1), TunnelPNoise = (int)std::ceil(6 / 6.1);
    // prefixLen: length of the shortest nonempty prefix whose units sum to >= h; total = that prefix's units
    auto prefix = [&](int h, int* total) -> int {
        int sum = 0;
        for (int i = 0; i < n_moduli; ++i) {
            sum += alch_modulus_units(moduli[i]);
            if (sum >= h) { if (total) *total = sum; return i + 1; }
        }
        return -1;
    };
    const int p = p_noise_out;
    const int lout = prefix(p + MinUnits, nullptr);                               // PNoise2Zq zqs p
    int tot_in = 0;
    const int lin = op == ALCH_OP_MUL ? prefix(p + MulPNoise + MinUnits, &tot_in)   // PreMul_: Units2CTPNoise (TotalUnits zqs (CTPNoise2Units (p :+ MulPNoise)))
                                      : prefix(p + TunnelPNoise + MinUnits, &tot_in);
    // KSPNoise, KSPNoise2Units: the reference defines it for TrivGad (+ Max32BitUnits) and BaseBGad 2 (+ 0) only.  BaseBGad 2^w is this
    // library's own rule, w - 1 more bits of digit in units of 6.1: + ceil((w - 1) / 6.1), which gives + 0 at w = 1 and reproduces
    // Max32BitUnits for a 30.5-bit digit.
    const int ks_units = p + KSAccumPNoise + (gw == 0 ? Max32BitUnits : (int)std::ceil((gw - 1) / 6.1));
    const int lh = prefix(ks_units, nullptr);
    if (lout < 0 || lin < 0 || lh < 0)
        return fail(ALCH_E_INVALID, "alch_select_limbs: the moduli do not hold enough noise units (PT2CT: \"You need more/bigger moduli!\")");
    if (L_in) *L_in = lin;
    if (L_hint) *L_hint = lh;
    if (L_out) *L_out = lout;
    if (p_noise_in) *p_noise_in = op == ALCH_OP_MUL ? tot_in - MinUnits : p + TunnelPNoise;
    return ALCH_OK;
} catch (...) { return abi_catch(); }

extern "C" int alch_host_root(uint32_t m, uint64_t q, uint64_t* psi, uint64_t* generator) try {
    if (m < 1 || q < 2) return fail(ALCH_E_INVALID, "alch_host_root: bad (m, q)");
    if (q < 3 || !h_is_prime(q)) return fail(ALCH_E_NOT_PRIME, "alch_host_root: q is not an odd prime");
    if ((q - 1) % m) return fail(ALCH_E_NO_CRT, "q is not 1 mod m");
    if (generator) *generator = h_smallest_generator(q);
    if (psi) *psi = h_root(q, m);
    return ALCH_OK;
} catch (...) { return abi_catch(); }

static int ring_create_impl(uint32_t m, int L, const uint64_t* q, bool nocrt, alch_ring** out) {
    if (!out) return fail(ALCH_E_INVALID, "alch_ring_create: null out");
    *out = nullptr;
    int logn = 0, word = 0;
    const bool gen = nocrt || !two_power_engine(m);
    GenHost gh;
    bool zdom = false;
    int rc = gen ? validate_gen_args(m, L, q, nocrt, gh, &word, &zdom) : validate_ring_args(m, L, q, &logn, &word);
    if (rc != ALCH_OK) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(ALCH_E_NO_DEVICE, "no HIP device: this backend has no CPU fallback");
    hipDeviceProp_t prop;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess)
        return fail(ALCH_E_NO_DEVICE, "cannot query HIP device");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(ALCH_E_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");

    alch_ring* r = new alch_ring();
    r->m = m;
    r->n = gen ? gh.n : m / 2;
    r->logn = logn;
    r->gen = gen;
    r->has_crt = !nocrt;
    r->zdom = zdom;
    r->gh = gh;
    r->L = L;
    r->word = word;
    for (int j = 0; j < L; ++j) r->q[j] = q[j];
    u64 qmin = ~0ull, qmax = 0;
    for (int j = 0; j < L; ++j) { qmin = std::min(qmin, q[j]); qmax = std::max(qmax, q[j]); }
    r->balanced = qmax > 0 && (qmax - 1) / 2 < qmin;
    r->q30 = r->word == 4 && qmax > 0 && qmax < ((u64)1 << 30);
    r->device = dev;
    hipError_t e = hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete r; return fail(ALCH_E_HIP, "hipStreamCreate failed"); }
    r->stream_owner = std::make_shared<StreamOwner>(r->stream, dev);
    if (hipEventCreate(&r->ev0) != hipSuccess || hipEventCreate(&r->ev1) != hipSuccess) { delete r; return fail(ALCH_E_HIP, "hipEventCreate failed"); }
    if (hipStreamCreateWithFlags(&r->aux, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&r->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&r->ev_join, hipEventDisableTiming) != hipSuccess) { delete r; return fail(ALCH_E_HIP, "aux stream/event creation failed"); }
    if (hipMalloc((void**)&r->ws_sum, sizeof(u64)) != hipSuccess) { delete r; return fail(ALCH_E_NOMEM, "hipMalloc failed"); }
    if (hipMalloc((void**)&r->d_flag, sizeof(int)) != hipSuccess) { alch_ring_destroy(r); return fail(ALCH_E_NOMEM, "hipMalloc failed"); }
    if (gen) rc = (word == 4) ? build_gen_ring<u32>(r, r->d32, r->g32) : build_gen_ring<u64>(r, r->d64, r->g64);
    else rc = (word == 4) ? build_dev_ring<u32>(r, r->d32) : build_dev_ring<u64>(r, r->d64);
    if (rc != ALCH_OK) { alch_ring_destroy(r); return rc; }
    *out = r;
    return ALCH_OK;
}

extern "C" int alch_ring_create(uint32_t m, int L, const uint64_t* q, alch_ring** out) try { return ring_create_impl(m, L, q, false, out); } catch (...) { return abi_catch(); }
extern "C" int alch_ring_create_nocrt(uint32_t m, int L, const uint64_t* q, alch_ring** out) try { return ring_create_impl(m, L, q, true, out); } catch (...) { return abi_catch(); }

static void wipe_rng_key(alch_ring* r) {
    volatile uint32_t* k = r->rng_key.k;           // volatile: the stores stay although the object dies next
    for (int i = 0; i < 8; ++i) k[i] = 0;
    r->rng_keyed = false;
}

extern "C" int alch_ring_destroy(alch_ring* r) try {
    if (!r) return ALCH_OK;
    ALCH_DEVICE_LOCK(r->device);
    (void)hipSetDevice(r->device);
    if (r->scratch) { alch_buf* b = r->scratch; r->scratch = nullptr; (void)hipFree(b->dptr); delete b; }
    (void)hipStreamSynchronize(r->stream);         // whichever stream it is: the null stream is a stream like any other
    for (auto& e : r->pool) (void)hipFree(e.second);
    r->pool.clear();
    for (auto& pn : r->pin) { if (pn.p) (void)hipHostFree(pn.p); if (pn.ev) (void)hipEventDestroy(pn.ev); pn = alch_ring::Pin(); }
    if (r->tables) (void)hipFree(r->tables);
    if (r->gen_tables) (void)hipFree(r->gen_tables);
    if (r->d_flag) (void)hipFree(r->d_flag);
    for (auto& e : r->ext) {
        if (e.second.pow_gather) (void)hipFree(e.second.pow_gather);
        if (e.second.coeffs) (void)hipFree(e.second.coeffs);
        if (e.second.slot_small) (void)hipFree(e.second.slot_small);
        if (e.second.fibres) (void)hipFree(e.second.fibres);
    }
    for (auto& e : r->autotab) (void)hipFree(e.second);
    if (r->tables_p) (void)hipFree(r->tables_p);
    for (Scratch* w : {&r->ws_auto, &r->ws_digits, &r->ws_in, &r->ws_full, &r->ws_lift, &r->ws_maxd, &r->ws_gauss, &r->ws_host}) w->release();
    if (r->ev_x) (void)hipEventDestroy(r->ev_x);
    if (r->ws_sum) (void)hipFree(r->ws_sum);
    if (r->ev0) (void)hipEventDestroy(r->ev0);
    if (r->ev1) (void)hipEventDestroy(r->ev1);
    if (r->ev_fork) (void)hipEventDestroy(r->ev_fork);
    for (int e = 0; e < 2; ++e) { if (r->ev_pa[e]) (void)hipEventDestroy(r->ev_pa[e]); if (r->ev_pb[e]) (void)hipEventDestroy(r->ev_pb[e]); }
    if (r->ev_join) (void)hipEventDestroy(r->ev_join);
    if (r->aux) { (void)hipStreamSynchronize(r->aux); (void)hipStreamDestroy(r->aux); }
    for (int e = 0; e < 2; ++e) {
        if (r->xs[e]) { (void)hipStreamSynchronize(r->xs[e]); (void)hipStreamDestroy(r->xs[e]); }
        if (r->ev_xs[e]) (void)hipEventDestroy(r->ev_xs[e]);
    }
    r->stream_owner.reset();                       // destroys the stream with its last user
    wipe_rng_key(r);
    delete r;
    return ALCH_OK;
} catch (...) { return abi_catch(); }

// The 32 key bytes (NULL: back to splitmix64), copied under the device lock: a sampler call in flight on another thread has either the
// old key or the new one, never a mixture.
extern "C" int alch_ring_set_rng_key(alch_ring* r, const void* key) try {
    if (!r) return fail(ALCH_E_INVALID, "null ring");
    ALCH_DEVICE_LOCK(r->device);
    wipe_rng_key(r);
    if (key) { r->rng_key = chacha::load_key(static_cast<const uint8_t*>(key)); r->rng_keyed = true; }
    return ALCH_OK;
} catch (...) { return abi_catch(); }

// No lock (as alch_ring_device): the Haskell host imports both `unsafe`, a call that must never wait.  One aligned word is read; a host
// that changes a ring's key or stream on one thread and asks for it on another orders the two itself.
extern "C" int alch_ring_rng(const alch_ring* r) try {
    if (!r) return fail(ALCH_E_INVALID, "null ring");
    return r->rng_keyed ? ALCH_RNG_CHACHA20 : ALCH_RNG_SPLITMIX;
} catch (...) { return abi_catch(); }

// The definition made callable (host only): the pairs (A, B) of positions x0 .. x0 + count - 1 of (key, nonce, domain).
extern "C" int alch_rng_words(const void* key, uint64_t nonce, unsigned domain, uint64_t x0, size_t count, uint64_t* out) try {
    if (!key || (!out && count)) return fail(ALCH_E_INVALID, "alch_rng_words: null pointer");
    if (domain >= chacha::DOMAINS) return fail(ALCH_E_INVALID, "alch_rng_words: the domain is a tag below 256");
    if (!chacha::range_ok(x0, count)) return fail(ALCH_E_INVALID, "alch_rng_words: positions end at 2^58");
    const chacha::Key K = chacha::load_key(static_cast<const uint8_t*>(key));
    u64 u[8];
    for (size_t i = 0; i < count; ++i) {
        const u64 x = x0 + i;
        if (i == 0 || chacha::slot(x) == 0) chacha::block(K, chacha::block_counter(domain, x), nonce, u);
        out[2 * i] = u[2 * chacha::slot(x)];
        out[2 * i + 1] = u[2 * chacha::slot(x) + 1];
    }
    volatile u64* w = u;                           // keystream of the caller's key: not left on the stack
    for (int i = 0; i < 8; ++i) w[i] = 0;
    return ALCH_OK;
} catch (...) { return abi_catch(); }

extern "C" int alch_ring_n(const alch_ring* r, uint32_t* n, int* L, int* word_bytes) try {
    if (!r) return fail(ALCH_E_INVALID, "null ring");
    if (n) *n = r->n;
    if (L) *L = r->L;
    if (word_bytes) *word_bytes = r->word;
    return ALCH_OK;
} catch (...) { return abi_catch(); }

extern "C" int alch_ring_set_stream(alch_ring* r, void* s) try {
    if (!r) return fail(ALCH_E_INVALID, "null ring");
    BIND(r);
    HIP_TRY(hipStreamSynchronize(r->stream));
    r->stream_owner.reset();
    r->stream = (hipStream_t)s;
    return ALCH_OK;
} catch (...) { return abi_catch(); }

extern "C" int alch_ring_set_option(alch_ring* r, const char* name, long value) try {
    if (!r || !name) return fail(ALCH_E_INVALID, "null argument");
    ALCH_DEVICE_LOCK(r->device);                                      // a call in flight on another thread reads the options under this lock
    const std::string k(name);
    if (k == "chunk") { if (value < 8) return fail(ALCH_E_INVALID, "chunk must be >= 8"); r->chunk = (size_t)value; }
    else if (k == "one_stream") r->one_stream = value != 0;
    else if (k == "pipe") r->pipe = value != 0;
    else if (k == "ks_map") r->opts.ks_map = value != 0;
    else if (k == "ks_rev") r->opts.ks_rev = value != 0;
    else if (k == "nstreams") { if (value < 1 || value > 4) return fail(ALCH_E_INVALID, "nstreams: 1 .. 4"); r->nstreams = (int)value; }
    else if (k == "q30") r->opts.q30 = value != 0;
    else if (k == "ks_grid") { if (value < 1) return fail(ALCH_E_INVALID, "ks_grid must be >= 1"); r->opts.ks_grid = (unsigned)value; }
    else if (k == "ti_grid") r->opts.ti_grid = (int)value;
    else if (k == "ti_split") { if (value < 0) return fail(ALCH_E_INVALID, "ti_split must be >= 0"); r->opts.ti_split = (int)value; }
    else if (k == "rs_lin") r->opts.rs_lin = value != 0;
    else if (k == "crt_half") r->opts.crt_half = value != 0;
    else if (k == "rs_half") r->opts.rs_half = value != 0;
    else if (k == "tunnel_ep") r->opts.tunnel_ep = value != 0;
    else if (k == "gen_fused") r->opts.gen_fused = value != 0;
    else if (k == "tunnel_mac") r->opts.tunnel_mac = value != 0;
    else if (k == "tunnel_fused") { if (value < 0 || (value != 0 && value != 2 && value != 4)) return fail(ALCH_E_INVALID, "tunnel_fused: 0 (composed), 2 or 4 (digits side by side)"); r->opts.tunnel_fused = (int)value; }
    else if (k == "gen_nt") {
        if (value != 0 && value != 128 && value != 256 && value != 512) return fail(ALCH_E_INVALID, "gen_nt must be 0 (by ring size), 128, 256 or 512");
        r->g32.nt = (int)value; r->g64.nt = (int)value;
    }
    else if (k == "split_fused") { if (value < 0 || value > 2) return fail(ALCH_E_INVALID, "split_fused: 0, 1 or 2"); r->opts.split_fused = (int)value; }
    else if (k == "scratch_mib") { if (value < 1 || value > 65536) return fail(ALCH_E_INVALID, "scratch_mib must be 1 .. 65536"); r->scratch_mib = (size_t)value; }
    else if (k == "rs_slots") { if (value < 1) return fail(ALCH_E_INVALID, "rs_slots must be >= 1"); r->rs_slots = (unsigned)value; }
    else if (k == "stream_dedicated") {
        // A new stream with an (all-ones) CU mask replaces the ring's: the HIP runtime gives such a stream a hardware queue of its own.
        // Ordinary streams share the runtime's pool of hardware queues (4 by default) by a rule that depends on how many streams the
        // process holds, so two "independent" streams land on ONE queue every other time and their kernels run one after the other
        // (measured with tools/queue_probe.py: the two sub-batches of the HomomRLWR pipeline at 44.7 k instead of 50.5 k pipelines/s
        // for every odd number of other rings alive; stream priorities do not separate them reliably either: 46 k every other time).
        // For hosts that run independent sub-batches side by side (alchemy_amd/ringround.py); every dedicated stream costs a
        // hardware queue, so it is an option, not the default of the hundreds of rings a Lol host creates.
        if (value != 1) return fail(ALCH_E_INVALID, "stream_dedicated: 1");
        BIND(r);
        if (++g_dedicated_streams > MAX_DEDICATED_STREAMS) {
            --g_dedicated_streams;
            return fail(ALCH_E_UNSUPPORTED, "stream_dedicated: " + std::to_string(MAX_DEDICATED_STREAMS) + " dedicated streams are alive in this process already "
                                            "(each holds a hardware queue; the ring keeps its ordinary stream)");
        }
        struct Undo { bool armed = true; ~Undo() { if (armed) --g_dedicated_streams; } } undo;       // any failure below gives the slot back
        HIP_TRY(hipStreamSynchronize(r->stream));
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, r->device));
        std::vector<uint32_t> mask((size_t)(prop.multiProcessorCount + 31) / 32, 0xffffffffu);
        if (prop.multiProcessorCount % 32) mask.back() = (1u << (prop.multiProcessorCount % 32)) - 1u;
        hipStream_t ns = nullptr;
        HIP_TRY(hipExtStreamCreateWithCUMask(&ns, (uint32_t)mask.size(), mask.data()));
        r->stream_owner = std::make_shared<StreamOwner>(ns, r->device, true);   // the old stream goes with its last user
        undo.armed = false;                                                      // the owner returns the slot when the stream dies
        r->stream = ns;
    }
    else return fail(ALCH_E_INVALID, "unknown option '" + k + "'");
    return ALCH_OK;
} catch (...) { return abi_catch(); }

extern "C" int alch_sync(alch_ring* r) try {
    if (!r) return fail(ALCH_E_INVALID, "null ring");
    BIND(r);
    HIP_TRY(hipStreamSynchronize(r->stream));
    return ALCH_OK;
} catch (...) { return abi_catch(); }

extern "C" int alch_timer_start(alch_ring* r) try {
    if (!r) return fail(ALCH_E_INVALID, "null ring");
    BIND(r);
    HIP_TRY(hipEventRecord(r->ev0, r->stream));
    return ALCH_OK;
} catch (...) { return abi_catch(); }

extern "C" int alch_timer_stop(alch_ring* r, float* ms) try {
    if (!r || !ms) return fail(ALCH_E_INVALID, "null argument");
    BIND(r);
    HIP_TRY(hipEventRecord(r->ev1, r->stream));
    HIP_TRY(hipEventSynchronize(r->ev1));
    HIP_TRY(hipEventElapsedTime(ms, r->ev0, r->ev1));
    return ALCH_OK;
} catch (...) { return abi_catch(); }

// ------------------------------------------------------------------------------------------------------
// helpers
// ------------------------------------------------------------------------------------------------------
// rings whose limb-polynomial does not fit one LDS-resident transform (k_crt_split); a general-index ring has logn = 0
static inline bool split_ring(const alch_ring* r) { return r->logn > (r->word == 4 ? 15 : 14); }
// f<W>(args) for the ring's word size
#define ALCH_BY_WORD(ringp, f, ...) ((ringp)->word == 4 ? f<u32>(__VA_ARGS__) : f<u64>(__VA_ARGS__))
static inline size_t elem_words(const alch_ring* r) { return (size_t)r->L * r->n; }
static inline size_t elem_bytes(const alch_ring* r) { return elem_words(r) * (size_t)r->word; }

int Scratch::reserve(size_t need) {
    if (bytes >= need) return ALCH_OK;
    release();
    if (hipMalloc(&p, need) != hipSuccess) return fail(ALCH_E_NOMEM, "hipMalloc(" + std::to_string(need) + ") failed");
    bytes = need;
    return ALCH_OK;
}

template <typename W> static const DevRing<W>& dev_ring(const alch_ring* r);
template <> const DevRing<u32>& dev_ring<u32>(const alch_ring* r) { return r->d32; }
template <> const DevRing<u64>& dev_ring<u64>(const alch_ring* r) { return r->d64; }

static hipError_t dispatch(int logn, const NttCall<u32>& c) {
    if (logn <= 9) return dispatch32_small(logn, c);
    if (logn <= 13) return dispatch32_mid(logn, c);
    if (logn == 14) return dispatch32_14(logn, c);
    if (logn == 15) return dispatch32_15(logn, c);
    return dispatch32_16(logn, c);
}
static hipError_t dispatch(int logn, const NttCall<u64>& c) {
    if (logn <= 11) return dispatch64_small(logn, c);
    if (logn <= 14) return dispatch64_big(logn, c);
    return dispatch64_15(logn, c);
}
// Queue one transform-engine / pass-engine launch: ALCH_OK, or ALCH_E_HIP with "<what> launch: <HIP's text>".
template <typename W>
static int launch(const alch_ring* r, const NttCall<W>& c, const char* what) {
    const hipError_t e = dispatch(r->logn, c);
    return e == hipSuccess ? ALCH_OK : fail(ALCH_E_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
}
template <typename W>
static int launch(const GenCall<W>& g, const char* what) {
    const hipError_t e = gen_dispatch(g);
    return e == hipSuccess ? ALCH_OK : fail(ALCH_E_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
}

template <typename W>
static int do_crt(alch_ring* r, void* data, size_t first_elem, size_t count, bool inverse, const void* src = nullptr,
                  const alch_ring* on = nullptr) {
    // src != null: transform src[first_elem ..) into data[first_elem ..) (LDS-resident sizes only)
    // on != null: queue on that ring's stream, whatever stream that is (the null stream included) -- the call is part of that ring's
    // pipeline; a ring, never a hipStream_t: a stream handle has no value that can stand for "not given"
    const hipStream_t stream = (on ? on : r)->stream;
    if (count == 0) return ALCH_OK;
    if (!r->has_crt) return fail(ALCH_E_NO_CRT, "this ring has no CRT basis (created with alch_ring_create_nocrt)");
    if (r->gen) {
        GenCall<W> g{};
        g.op = inverse ? GEN_CRTINV : GEN_CRT;
        g.ring = &dev_ring<W>(r);
        g.gen = &gen_dev<W>(r);
        g.stream = stream;
        g.data = reinterpret_cast<W*>(data);
        g.src = reinterpret_cast<const W*>(src);
        const size_t polys = count * (size_t)r->L;
        for (size_t done = 0; done < polys;) {
            const size_t now = std::min<size_t>(polys - done, (size_t)1 << 30);
            g.first_poly = first_elem * (size_t)r->L + done;
            g.npoly = now;
            if (int rc = launch(g, "general-index crt")) return rc;
            done += now;
        }
        return ALCH_OK;
    }
    NttCall<W> c{};
    c.src = reinterpret_cast<const W*>(src);
    c.op = inverse ? OP_CRTINV : OP_CRT;
    c.ring = &dev_ring<W>(r);
    c.stream = stream;
    c.data = reinterpret_cast<W*>(data);
    const size_t polys = count * (size_t)r->L;
    // grids are 32-bit: split very large batches
    size_t done = 0;
    while (done < polys) {
        size_t now = std::min<size_t>(polys - done, (size_t)1 << 30);
        c.first_poly = first_elem * (size_t)r->L + done;
        c.npoly = now;
        if (int rc = launch(r, c, "crt")) return rc;
        done += now;
    }
    return ALCH_OK;
}

// Transformed copies of `srcs` (count_each elements each) in consecutive regions of dst.  The split transforms (n = 2^16 / 64-bit 2^15)
// work in place only: one copy per source, then ONE transform over all of them; every other ring transforms out of place from each source.
template <typename W>
static int crt_into(alch_ring* r, void* dst, std::initializer_list<const void*> srcs, size_t count_each, bool inverse, const alch_ring* on = nullptr) {
    const size_t bytes = count_each * elem_bytes(r);
    char* d = reinterpret_cast<char*>(dst);
    for (const void* src : srcs) {
        if (split_ring(r)) HIP_TRY(hipMemcpyAsync(d, src, bytes, hipMemcpyDeviceToDevice, (on ? on : r)->stream));
        else if (int rc = do_crt<W>(r, d, 0, count_each, inverse, src, on)) return rc;
        d += bytes;
    }
    return split_ring(r) ? do_crt<W>(r, dst, 0, srcs.size() * count_each, inverse, nullptr, on) : ALCH_OK;
}

static int buf_crt(alch_buf* b, size_t first, size_t count, bool inverse) {
    if (!b) return fail(ALCH_E_INVALID, "null buffer");
    if (!range_ok(first, count, b->n_elems)) return fail(ALCH_E_INVALID, "element range out of bounds");
    alch_ring* r = b->ring;
    BIND(r);
    return ALCH_BY_WORD(r, do_crt, r, b->dptr, first, count, inverse);
}

// ------------------------------------------------------------------------------------------------------
// device buffers
// ------------------------------------------------------------------------------------------------------
extern "C" int alch_buf_alloc(alch_ring* r, size_t n_elems, alch_buf** out) try {
    if (!r || !out || n_elems == 0) return fail(ALCH_E_INVALID, "alch_buf_alloc: bad argument");
    if (n_elems > (size_t)-1 / elem_bytes(r)) return fail(ALCH_E_INVALID, "alch_buf_alloc: n_elems * element size overflows size_t");
    BIND(r);
    const size_t bytes = n_elems * elem_bytes(r);
    if (bytes <= POOL_MAX_BUF) {
        std::lock_guard<std::mutex> lk(r->pool_mu);
        for (size_t i = r->pool.size(); i-- > 0;)
            if (r->pool[i].first == n_elems) {                     // stream-ordered reuse (see alch_ring::pool)
                void* p = r->pool[i].second;
                r->pool[i] = r->pool.back();
                r->pool.pop_back();
                r->pool_bytes -= bytes;
                *out = new alch_buf{r, n_elems, p};
                return ALCH_OK;
            }
    }
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
        // parked buffers may be what exhausts the device: release them and try once more
        std::vector<std::pair<size_t, void*>> parked;
        { std::lock_guard<std::mutex> lk(r->pool_mu); parked.swap(r->pool); r->pool_bytes = 0; }
        if (!parked.empty()) {
            (void)hipStreamSynchronize(r->stream);
            for (auto& e : parked) (void)hipFree(e.second);
            if (hipMalloc(&p, bytes) != hipSuccess) p = nullptr;
        }
        if (!p) return fail(ALCH_E_NOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes failed");
    }
    *out = new alch_buf{r, n_elems, p};
    return ALCH_OK;
} catch (...) { return abi_catch(); }

extern "C" int alch_buf_view(const alch_buf* parent, size_t first, size_t count, alch_buf** out) try {
    if (!parent || !out || count == 0) return fail(ALCH_E_INVALID, "alch_buf_view: bad argument");
    if (!range_ok(first, count, parent->n_elems)) return fail(ALCH_E_INVALID, "element range out of bounds");
    alch_buf* v = new alch_buf{parent->ring, count, reinterpret_cast<char*>(parent->dptr) + first * elem_bytes(parent->ring)};
    v->view = true;
    *out = v;
    return ALCH_OK;
} catch (...) { return abi_catch(); }

extern "C" int alch_buf_free(alch_buf* b) try {
    if (!b) return ALCH_OK;
    if (b->view) { delete b; return ALCH_OK; }                      // an alias owns nothing
    alch_ring* r = b->ring;
    const size_t bytes = b->n_elems * elem_bytes(r);
    if (bytes <= POOL_MAX_BUF) {
        std::lock_guard<std::mutex> lk(r->pool_mu);
        if (r->pool_bytes + bytes <= POOL_CAP) {
            r->pool.emplace_back(b->n_elems, b->dptr);             // no synchronisation: reuse is ordered on the ring's stream
            r->pool_bytes += bytes;
            delete b;
            return ALCH_OK;
        }
    }
    (void)hipSetDevice(r->device);
    (void)hipStreamSynchronize(r->stream);
    (void)hipFree(b->dptr);
    delete b;
    return ALCH_OK;
} catch (...) { return abi_catch(); }

extern "C" int alch_buf_elems(const alch_buf* b, size_t* n) try {
    if (!b || !n) return fail(ALCH_E_INVALID, "null argument");
    *n = b->n_elems;
    return ALCH_OK;
} catch (...) { return abi_catch(); }

extern "C" int alch_buf_device_ptr(const alch_buf* b, void** ptr, size_t* bytes) try {
    if (!b || !ptr) return fail(ALCH_E_INVALID, "null argument");
    *ptr = b->dptr;
    if (bytes) *bytes = b->n_elems * elem_bytes(b->ring);
    return ALCH_OK;
} catch (...) { return abi_catch(); }

extern "C" int alch_buf_ring(const alch_buf* b, alch_ring** ring) try {
    if (!b || !ring) return fail(ALCH_E_INVALID, "null argument");
    *ring = b->ring;
    return ALCH_OK;
} catch (...) { return abi_catch(); }

extern "C" int alch_ring_device(const alch_ring* r, int* device, void** hip_stream) try {
    if (!r) return fail(ALCH_E_INVALID, "null ring");
    if (device) *device = r->device;
    if (hip_stream) *hip_stream = (void*)r->stream;
    return ALCH_OK;
} catch (...) { return abi_catch(); }

template <typename W>
static int do_transfer(alch_ring* r, void* dev, size_t count, int64_t* host, bool to_device) {
    ALCH_REQUIRE_DEVICE_LOCK(r, "do_transfer");                       // ws_host, pin[], pin_next
    const size_t bytes = count * elem_words(r) * sizeof(int64_t);
    int rc = r->ws_host.reserve(bytes);
    if (rc != ALCH_OK) return rc;
    int64_t* stage = reinterpret_cast<int64_t*>(r->ws_host.p);
    const size_t total = count * elem_words(r);
    if (bytes <= PIN_MAX) {
        // small transfer (the per-Tensor-call path moves one ring element at a time): through a pinned slot
        alch_ring::Pin& pn = r->pin[r->pin_next];
        r->pin_next = (r->pin_next + 1) % 4;
        if (pn.busy) { HIP_TRY(hipEventSynchronize(pn.ev)); pn.busy = false; }     // the slot's last upload has left it (long ago, normally)
        if (pn.bytes < bytes) {
            if (pn.p) { (void)hipHostFree(pn.p); pn.p = nullptr; pn.bytes = 0; }
            if (hipHostMalloc(&pn.p, bytes, hipHostMallocDefault) != hipSuccess) return fail(ALCH_E_NOMEM, "hipHostMalloc(" + std::to_string(bytes) + ") failed");
            pn.bytes = bytes;
        }
        if (!pn.ev) HIP_TRY(hipEventCreateWithFlags(&pn.ev, hipEventDisableTiming));
        if (to_device) {
            memcpy(pn.p, host, bytes);                             // the caller's buffer is consumed here: no synchronisation needed
            HIP_TRY(hipMemcpyAsync(stage, pn.p, bytes, hipMemcpyHostToDevice, r->stream));
            hipLaunchKernelGGL((k_transpose<W, true>), dim3(ew_grid(total)), dim3(256), 0, r->stream, dev_ring<W>(r),
                               reinterpret_cast<W*>(dev), stage, count);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(pn.ev, r->stream));
            pn.busy = true;
        } else {
            hipLaunchKernelGGL((k_transpose<W, false>), dim3(ew_grid(total)), dim3(256), 0, r->stream, dev_ring<W>(r),
                               reinterpret_cast<W*>(dev), stage, count);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(pn.p, stage, bytes, hipMemcpyDeviceToHost, r->stream));
            HIP_TRY(hipStreamSynchronize(r->stream));              // the one synchronisation of a download
            memcpy(host, pn.p, bytes);
        }
        return ALCH_OK;
    }
    if (to_device) {
        HIP_TRY(hipMemcpyAsync(stage, host, bytes, hipMemcpyHostToDevice, r->stream));
        hipLaunchKernelGGL((k_transpose<W, true>), dim3(ew_grid(total)), dim3(256), 0, r->stream, dev_ring<W>(r),
                           reinterpret_cast<W*>(dev), stage, count);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(r->stream));      // host buffer is caller-owned: do not retain it
    } else {
        hipLaunchKernelGGL((k_transpose<W, false>), dim3(ew_grid(total)), dim3(256), 0, r->stream, dev_ring<W>(r),
                           reinterpret_cast<W*>(dev), stage, count);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(host, stage, bytes, hipMemcpyDeviceToHost, r->stream));
        HIP_TRY(hipStreamSynchronize(r->stream));
    }
    return ALCH_OK;
}

static int transfer(alch_ring* r, void* dev_base, size_t first, size_t count, int64_t* host, bool to_device) {
    BIND(r);
    // bounded staging: move at most 64 MiB of int64 at a time
    const size_t per = std::max<size_t>(1, ((size_t)64 << 20) / (elem_words(r) * sizeof(int64_t)));
    size_t done = 0;
    while (done < count) {
        const size_t now = std::min(per, count - done);
        char* dev = reinterpret_cast<char*>(dev_base) + (first + done) * elem_bytes(r);
        int64_t* h = host + done * elem_words(r);
        int rc = ALCH_BY_WORD(r, do_transfer, r, dev, now, h, to_device);
        if (rc != ALCH_OK) return rc;
        done += now;
    }
    return ALCH_OK;
}

extern "C" int alch_buf_upload(alch_buf* b, size_t first, size_t count, const int64_t* host) try {
    if (!b || !host) return fail(ALCH_E_INVALID, "null argument");
    if (!range_ok(first, count, b->n_elems)) return fail(ALCH_E_INVALID, "element range out of bounds");
    return transfer(b->ring, b->dptr, first, count, const_cast<int64_t*>(host), true);
} catch (...) { return abi_catch(); }

extern "C" int alch_buf_download(const alch_buf* b, size_t first, size_t count, int64_t* host) try {
    if (!b || !host) return fail(ALCH_E_INVALID, "null argument");
    if (!range_ok(first, count, b->n_elems)) return fail(ALCH_E_INVALID, "element range out of bounds");
    return transfer(b->ring, b->dptr, first, count, host, false);
} catch (...) { return abi_catch(); }

extern "C" int alch_buf_fill_uniform(alch_buf* b, uint64_t seed) try {
    if (!b) return fail(ALCH_E_INVALID, "null buffer");
    alch_ring* r = b->ring;
    BIND(r);
    const size_t words = b->n_elems * elem_words(r);
    if (r->word == 4)
        hipLaunchKernelGGL((k_fill_uniform<u32>), dim3(ew_grid(words)), dim3(256), 0, r->stream, r->d32, (u32*)b->dptr, words, seed);
    else
        hipLaunchKernelGGL((k_fill_uniform<u64>), dim3(ew_grid(words)), dim3(256), 0, r->stream, r->d64, (u64*)b->dptr, words, seed);
    HIP_TRY(hipGetLastError());
    return ALCH_OK;
} catch (...) { return abi_catch(); }

extern "C" int alch_buf_crt(alch_buf* b, size_t first, size_t count) try { return buf_crt(b, first, count, false); } catch (...) { return abi_catch(); }
extern "C" int alch_buf_crtinv(alch_buf* b, size_t first, size_t count) try { return buf_crt(b, first, count, true); } catch (...) { return abi_catch(); }

template <typename W, int OP>
static int do_pointwise(alch_ring* r, void* dst, const void* a, const void* b, size_t count) {
    const size_t words = count * elem_words(r);
    if (r->n % Vec4<W>::LANES)
        hipLaunchKernelGGL((k_pointwise_scalar<W, OP>), dim3(ew_grid(words)), dim3(256), 0, r->stream, dev_ring<W>(r),
                           (W*)dst, (const W*)a, (const W*)b, words);
    else
    hipLaunchKernelGGL((k_pointwise<W, OP>), dim3(ew_grid(words / Vec4<W>::LANES)), dim3(256), 0, r->stream, dev_ring<W>(r),
                       (W*)dst, (const W*)a, (const W*)b, words);
    HIP_TRY(hipGetLastError());
    return ALCH_OK;
}

static int buf_pointwise(alch_buf* dst, const alch_buf* a, const alch_buf* b, size_t count, int op) {
    if (!dst || !a || !b) return fail(ALCH_E_INVALID, "null buffer");
    if (a->ring != dst->ring || b->ring != dst->ring) return fail(ALCH_E_INVALID, "buffers belong to different rings");
    if (count > dst->n_elems || count > a->n_elems || count > b->n_elems) return fail(ALCH_E_INVALID, "count out of bounds");
    alch_ring* r = dst->ring;
    const size_t bytes = count * elem_bytes(r);
    if (count && (shifted_overlap(dst->dptr, bytes, a->dptr, bytes) || shifted_overlap(dst->dptr, bytes, b->dptr, bytes)))
        return fail(ALCH_E_INVALID, std::string(op == PW_MUL ? "alch_buf_mul" : op == PW_ADD ? "alch_buf_add" : "alch_buf_sub") +
                                        ": dst overlaps an operand without starting where it starts");
    BIND(r);
    if (!r->has_crt && op == PW_MUL) return fail(ALCH_E_NO_CRT, "pointwise products need the CRT basis; this ring has none");
    if (r->word == 4) {
        if (op == PW_MUL) return do_pointwise<u32, PW_MUL>(r, dst->dptr, a->dptr, b->dptr, count);
        if (op == PW_ADD) return do_pointwise<u32, PW_ADD>(r, dst->dptr, a->dptr, b->dptr, count);
        return do_pointwise<u32, PW_SUB>(r, dst->dptr, a->dptr, b->dptr, count);
    }
    if (op == PW_MUL) return do_pointwise<u64, PW_MUL>(r, dst->dptr, a->dptr, b->dptr, count);
    if (op == PW_ADD) return do_pointwise<u64, PW_ADD>(r, dst->dptr, a->dptr, b->dptr, count);
    return do_pointwise<u64, PW_SUB>(r, dst->dptr, a->dptr, b->dptr, count);
}

extern "C" int alch_buf_mul(alch_buf* d, const alch_buf* a, const alch_buf* b, size_t count) try { return buf_pointwise(d, a, b, count, PW_MUL); } catch (...) { return abi_catch(); }
extern "C" int alch_buf_add(alch_buf* d, const alch_buf* a, const alch_buf* b, size_t count) try { return buf_pointwise(d, a, b, count, PW_ADD); } catch (...) { return abi_catch(); }
extern "C" int alch_buf_sub(alch_buf* d, const alch_buf* a, const alch_buf* b, size_t count) try { return buf_pointwise(d, a, b, count, PW_SUB); } catch (...) { return abi_catch(); }

static int buf_checksum(const alch_buf* b, size_t first, size_t count, uint64_t position, uint64_t* sum) {
    if (!b || !sum) return fail(ALCH_E_INVALID, "null argument");
    if (!range_ok(first, count, b->n_elems)) return fail(ALCH_E_INVALID, "element range out of bounds");
    alch_ring* r = b->ring;
    BIND(r);
    const size_t words = count * elem_words(r);
    const char* base = reinterpret_cast<const char*>(b->dptr) + first * elem_bytes(r);
    HIP_TRY(hipMemsetAsync(r->ws_sum, 0, sizeof(u64), r->stream));
    if (r->word == 4) hipLaunchKernelGGL((k_checksum<u32>), dim3(ew_grid(words)), dim3(256), 0, r->stream, (const u32*)base, words, r->ws_sum, (u64)position * elem_words(r));
    else hipLaunchKernelGGL((k_checksum<u64>), dim3(ew_grid(words)), dim3(256), 0, r->stream, (const u64*)base, words, r->ws_sum, (u64)position * elem_words(r));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(sum, r->ws_sum, sizeof(u64), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return ALCH_OK;
}

extern "C" int alch_buf_checksum(const alch_buf* b, size_t first, size_t count, uint64_t* sum) try { return buf_checksum(b, first, count, 0, sum); } catch (...) { return abi_catch(); }
extern "C" int alch_buf_checksum_at(const alch_buf* b, size_t first, size_t count, uint64_t position, uint64_t* sum) try { return buf_checksum(b, first, count, position, sum); } catch (...) { return abi_catch(); }

// ------------------------------------------------------------------------------------------------------
// host-buffer Tensor methods: stage one element through a scratch device buffer
// ------------------------------------------------------------------------------------------------------
// The host-buffer Tensor methods stage their operands through a per-ring scratch array that is kept between
// calls (no hipMalloc / hipFree per ring element); it only ever grows.
struct ScratchBuf {
    alch_buf* b = nullptr;
};
// The caller holds the device lock from here until it has finished with the element: a second thread's request may replace it
// (alch_buf_free of the old one), and its upload would land on the words this one is about to download.
static int scratch_get(alch_ring* r, size_t n_elems, alch_buf** out) {
    ALCH_REQUIRE_DEVICE_LOCK(r, "scratch_get");
    if (r->scratch && r->scratch->n_elems >= n_elems) { *out = r->scratch; return ALCH_OK; }
    if (r->scratch) { alch_buf* old = r->scratch; r->scratch = nullptr; alch_buf_free(old); }
    int rc = alch_buf_alloc(r, n_elems, &r->scratch);
    if (rc != ALCH_OK) return rc;
    *out = r->scratch;
    return ALCH_OK;
}

static int host_unary(alch_ring* r, int64_t* data, int which) {
    if (!r || !data) return fail(ALCH_E_INVALID, "null argument");
    BIND(r);
    ScratchBuf s;
    int rc = scratch_get(r, 1, &s.b);
    if (rc != ALCH_OK) return rc;
    if ((rc = alch_buf_upload(s.b, 0, 1, data)) != ALCH_OK) return rc;
    if ((rc = buf_crt(s.b, 0, 1, which == 1)) != ALCH_OK) return rc;
    return alch_buf_download(s.b, 0, 1, data);
}

extern "C" int alch_crt(alch_ring* r, int64_t* data) try { return host_unary(r, data, 0); } catch (...) { return abi_catch(); }
extern "C" int alch_crtinv(alch_ring* r, int64_t* data) try { return host_unary(r, data, 1); } catch (...) { return abi_catch(); }

static int host_binary(alch_ring* r, int64_t* a, const int64_t* b, int op) {
    if (!r || !a || !b) return fail(ALCH_E_INVALID, "null argument");
    BIND(r);
    ScratchBuf s;
    int rc = scratch_get(r, 2, &s.b);
    if (rc != ALCH_OK) return rc;
    if ((rc = alch_buf_upload(s.b, 0, 1, a)) != ALCH_OK) return rc;
    if ((rc = alch_buf_upload(s.b, 1, 1, b)) != ALCH_OK) return rc;
    alch_buf second{r, 1, reinterpret_cast<char*>(s.b->dptr) + elem_bytes(r)};
    if ((rc = buf_pointwise(s.b, s.b, &second, 1, op)) != ALCH_OK) return rc;
    return alch_buf_download(s.b, 0, 1, a);
}

extern "C" int alch_mul(alch_ring* r, int64_t* a, const int64_t* b) try { return host_binary(r, a, b, PW_MUL); } catch (...) { return abi_catch(); }
extern "C" int alch_add(alch_ring* r, int64_t* a, const int64_t* b) try { return host_binary(r, a, b, PW_ADD); } catch (...) { return abi_catch(); }
extern "C" int alch_sub(alch_ring* r, int64_t* a, const int64_t* b) try { return host_binary(r, a, b, PW_SUB); } catch (...) { return abi_catch(); }

template <typename W>
static int scal_to_mont(const alch_ring* r, const uint64_t* s, int power_of_R, Scal<W>& out) {
    // out[j] = s[j] * R^power mod q_j  (s == NULL means 1)
    const int bits = 8 * (int)sizeof(W);
    for (int j = 0; j < MAXL; ++j) out.v[j] = 0;
    for (int j = 0; j < r->L; ++j) {
        const u64 q = r->q[j];
        u64 v = s ? s[j] % q : 1;
        const u64 r1 = h_powmod(2, (u64)bits, q);
        for (int p = 0; p < power_of_R; ++p) v = h_mulmod(v, r1, q);
        out.v[j] = (W)v;
    }
    return ALCH_OK;
}

template <typename W>
static int do_scale(alch_ring* r, void* dst, const void* src, size_t count, const uint64_t* s) {
    if (!r->has_crt) return fail(ALCH_E_UNSUPPORTED, "scalar products are implemented for rings with Montgomery constants (prime moduli) only");
    Scal<W> sm;
    scal_to_mont<W>(r, s, 1, sm);
    const size_t words = count * elem_words(r);
    ALCH_LAUNCH_VW(k_scale, r, words, r->stream, dev_ring<W>(r), (W*)dst, (const W*)src, words, sm);
    HIP_TRY(hipGetLastError());
    return ALCH_OK;
}

extern "C" int alch_scale(alch_ring* r, int64_t* a, const uint64_t* s) try {
    if (!r || !a || !s) return fail(ALCH_E_INVALID, "null argument");
    BIND(r);
    ScratchBuf t;
    int rc = scratch_get(r, 1, &t.b);
    if (rc != ALCH_OK) return rc;
    if ((rc = alch_buf_upload(t.b, 0, 1, a)) != ALCH_OK) return rc;
    rc = ALCH_BY_WORD(r, do_scale, r, t.b->dptr, t.b->dptr, 1, s);
    if (rc != ALCH_OK) return rc;
    return alch_buf_download(t.b, 0, 1, a);
} catch (...) { return abi_catch(); }

// mulG / divG / l / lInv on one host ring element: staged through the per-ring scratch element.
static int buf_mulg_divg(alch_buf* b, size_t first, size_t count, int basis, bool divide);
static int buf_l(alch_buf* b, size_t first, size_t count, bool inverse);
static int host_g(alch_ring* r, int64_t* a, int basis, int which /* 0 mulG, 1 divG, 2 l, 3 lInv */) {
    if (!r || !a) return fail(ALCH_E_INVALID, "null argument");
    if (basis == ALCH_BASIS_CRT && !r->has_crt) return fail(ALCH_E_NO_CRT, "this ring has no CRT basis");
    if (!r->gen || r->gh.rad == 1) return ALCH_OK;                    // two-power index: g = 1, L = identity
    BIND(r);
    ScratchBuf s;
    int rc = scratch_get(r, 1, &s.b);
    if (rc != ALCH_OK) return rc;
    if ((rc = alch_buf_upload(s.b, 0, 1, a)) != ALCH_OK) return rc;
    if (which == 0) rc = buf_mulg_divg(s.b, 0, 1, basis, false);
    else if (which == 1) rc = buf_mulg_divg(s.b, 0, 1, basis, true);
    else rc = buf_l(s.b, 0, 1, which == 3);
    if (rc != ALCH_OK) return rc;                                     // includes ALCH_NOT_DIVISIBLE: the host data stay untouched
    return alch_buf_download(s.b, 0, 1, a);
}
extern "C" int alch_mulg_pow(alch_ring* r, int64_t* a) try { return host_g(r, a, ALCH_BASIS_POW, 0); } catch (...) { return abi_catch(); }
extern "C" int alch_mulg_dec(alch_ring* r, int64_t* a) try { return host_g(r, a, ALCH_BASIS_DEC, 0); } catch (...) { return abi_catch(); }
extern "C" int alch_mulg_crt(alch_ring* r, int64_t* a) try { return host_g(r, a, ALCH_BASIS_CRT, 0); } catch (...) { return abi_catch(); }
extern "C" int alch_divg_pow(alch_ring* r, int64_t* a) try { return host_g(r, a, ALCH_BASIS_POW, 1); } catch (...) { return abi_catch(); }
extern "C" int alch_divg_dec(alch_ring* r, int64_t* a) try { return host_g(r, a, ALCH_BASIS_DEC, 1); } catch (...) { return abi_catch(); }
extern "C" int alch_divg_crt(alch_ring* r, int64_t* a) try { return host_g(r, a, ALCH_BASIS_CRT, 1); } catch (...) { return abi_catch(); }
extern "C" int alch_l(alch_ring* r, int64_t* a) try { return host_g(r, a, ALCH_BASIS_POW, 2); } catch (...) { return abi_catch(); }
extern "C" int alch_linv(alch_ring* r, int64_t* a) try { return host_g(r, a, ALCH_BASIS_POW, 3); } catch (...) { return abi_catch(); }

extern "C" int alch_decompose_triv(alch_ring* r, const int64_t* c_pow, int64_t* digits) try {
    if (!r || !c_pow || !digits) return fail(ALCH_E_INVALID, "null argument");
    BIND(r);
    ScratchBuf s;
    int rc = scratch_get(r, 1 + (size_t)r->L, &s.b);
    if (rc != ALCH_OK) return rc;
    if ((rc = alch_buf_upload(s.b, 0, 1, c_pow)) != ALCH_OK) return rc;
    char* dig = reinterpret_cast<char*>(s.b->dptr) + elem_bytes(r);
    const size_t total = (size_t)r->L * elem_words(r);
    if (r->word == 4) hipLaunchKernelGGL((k_decompose_triv<u32>), dim3(ew_grid(total)), dim3(256), 0, r->stream, r->d32, (const u32*)s.b->dptr, (u32*)dig, r->balanced ? 1 : 0);
    else hipLaunchKernelGGL((k_decompose_triv<u64>), dim3(ew_grid(total)), dim3(256), 0, r->stream, r->d64, (const u64*)s.b->dptr, (u64*)dig, r->balanced ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return alch_buf_download(s.b, 1, (size_t)r->L, digits);
} catch (...) { return abi_catch(); }

// The one predicate on gadget codes (hint_gadget.hpp): 0 TrivGad, w >= 1 BaseBGad 2^w, -1 unknown.
using hintgad::gadget_width;

// BaseBGad 2^w layout: limb i owns ceil(ceil(log2 q_i) / w) digits starting at first[i]; returns their total.
static int base2_layout(const alch_ring* r, Scal<u32>& first, Scal<u32>& kd, u32 w) {
    int D = 0;
    for (int j = 0; j < MAXL; ++j) { first.v[j] = 0; kd.v[j] = 0; }
    for (int i = 0; i < r->L; ++i) {
        const int k = (int)hintgad::digits_pow2(r->q[i], w);
        first.v[i] = (u32)D;
        kd.v[i] = (u32)k;
        D += k;
    }
    return D;
}

// gadget: a code gadget_width accepts.
static int gadget_digits(const alch_ring* r, int gadget) {
    const int w = gadget_width(gadget);
    if (w == 0) return r->L;
    Scal<u32> f, k;
    return base2_layout(r, f, k, (u32)w);
}

// k_decompose_base2 for `ny` elements on the ring's stream: the base-2 instantiation for w = 1, the closed form above it.
template <typename W>
static void launch_decompose_baseb(alch_ring* r, hipStream_t stream, const DevRing<W>& R, unsigned ny, const W* src, W* dst,
                                   const Scal<u32>& first, const Scal<u32>& kd, u32 D, u32 w) {
    const dim3 grid(ew_grid(elem_words(r)), ny);
    if (w > 1) hipLaunchKernelGGL((k_decompose_base2<W, true>), grid, dim3(256), 0, stream, R, src, dst, first, kd, D, w);
    else hipLaunchKernelGGL((k_decompose_base2<W, false>), grid, dim3(256), 0, stream, R, src, dst, first, kd, D, w);
}

static int decompose_baseb(alch_ring* r, u32 w, const int64_t* c_pow, int64_t* digits, int* n_digits) {
    Scal<u32> first, kd;
    const int D = base2_layout(r, first, kd, w);
    if (n_digits) *n_digits = D;
    if (!digits) return ALCH_OK;
    if (!c_pow) return fail(ALCH_E_INVALID, "null argument");
    BIND(r);                                                          // the n_digits-only query above reads immutable members
    ScratchBuf s;
    int rc = scratch_get(r, 1 + (size_t)D, &s.b);
    if (rc != ALCH_OK) return rc;
    if ((rc = alch_buf_upload(s.b, 0, 1, c_pow)) != ALCH_OK) return rc;
    char* dig = reinterpret_cast<char*>(s.b->dptr) + elem_bytes(r);
    if (r->word == 4) launch_decompose_baseb<u32>(r, r->stream, r->d32, 1, (const u32*)s.b->dptr, (u32*)dig, first, kd, (u32)D, w);
    else launch_decompose_baseb<u64>(r, r->stream, r->d64, 1, (const u64*)s.b->dptr, (u64*)dig, first, kd, (u32)D, w);
    HIP_TRY(hipGetLastError());
    return alch_buf_download(s.b, 1, (size_t)D, digits);
}

extern "C" int alch_decompose_base2(alch_ring* r, const int64_t* c_pow, int64_t* digits, int* n_digits) try {
    if (!r) return fail(ALCH_E_INVALID, "null ring");
    return decompose_baseb(r, 1, c_pow, digits, n_digits);
} catch (...) { return abi_catch(); }

extern "C" int alch_decompose_baseb(alch_ring* r, int gadget, const int64_t* c_pow, int64_t* digits, int* n_digits) try {
    if (!r) return fail(ALCH_E_INVALID, "alch_decompose_baseb: null ring");
    const int w = gadget_width(gadget);
    if (w < 1) return fail(ALCH_E_INVALID, "alch_decompose_baseb: unknown gadget (a BaseBGad code: ALCH_GAD_BASE2 or ALCH_GAD_BASEPOW2(1 .. 16))");
    return decompose_baseb(r, (u32)w, c_pow, digits, n_digits);
} catch (...) { return abi_catch(); }

extern "C" int alch_gadget_digits(const alch_ring* r, int gadget, int* D) try {
    if (!r || !D) return fail(ALCH_E_INVALID, "alch_gadget_digits: null argument");
    if (gadget_width(gadget) < 0) return fail(ALCH_E_INVALID, "alch_gadget_digits: unknown gadget");
    *D = gadget_digits(r, gadget);
    return ALCH_OK;
} catch (...) { return abi_catch(); }

// ------------------------------------------------------------------------------------------------------
// hint
// ------------------------------------------------------------------------------------------------------
static int hint_from_device(alch_ring* r, int gadget, const void* src_crt, alch_hint** out) {
    BIND(r);
    if (gadget_width(gadget) < 0) return fail(ALCH_E_INVALID, "alch_hint_load / alch_hint_from_buf: unknown gadget");
    const int digits = gadget_digits(r, gadget);
    const size_t elems = 2 * (size_t)digits;
    void* p = nullptr;
    if (hipMalloc(&p, elems * elem_bytes(r)) != hipSuccess) return fail(ALCH_E_NOMEM, "hipMalloc(hint) failed");
    // Montgomery form: multiply by R^2 under mont_mul  -> x * R
    int rc;
    if (r->word == 4) {
        Scal<u32> sm; scal_to_mont<u32>(r, nullptr, 2, sm);
        const size_t words = elems * elem_words(r);
        hipLaunchKernelGGL((k_scale<u32>), dim3(ew_grid(words)), dim3(256), 0, r->stream, r->d32, (u32*)p, (const u32*)src_crt, words, sm);
    } else {
        Scal<u64> sm; scal_to_mont<u64>(r, nullptr, 2, sm);
        const size_t words = elems * elem_words(r);
        hipLaunchKernelGGL((k_scale<u64>), dim3(ew_grid(words)), dim3(256), 0, r->stream, r->d64, (u64*)p, (const u64*)src_crt, words, sm);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { (void)hipFree(p); return fail(ALCH_E_HIP, std::string("hint conversion: ") + hipGetErrorString(e)); }
    rc = ALCH_OK;
    *out = new alch_hint{r, gadget, digits, p};
    return rc;
}

extern "C" int alch_buf_scale(alch_buf* dst, const alch_buf* src, size_t count, const uint64_t* s) try {
    if (!dst || !src || !s) return fail(ALCH_E_INVALID, "null argument");
    if (dst->ring != src->ring) return fail(ALCH_E_INVALID, "buffers belong to different rings");
    if (count > dst->n_elems || count > src->n_elems) return fail(ALCH_E_INVALID, "count out of bounds");
    alch_ring* r = dst->ring;
    if (count && shifted_overlap(dst->dptr, count * elem_bytes(r), src->dptr, count * elem_bytes(r)))
        return fail(ALCH_E_INVALID, "alch_buf_scale: dst overlaps src without starting where it starts");
    BIND(r);
    return ALCH_BY_WORD(r, do_scale, r, dst->dptr, src->dptr, count, s);
} catch (...) { return abi_catch(); }

extern "C" int alch_buf_decompose_triv(const alch_buf* src, size_t src_index, alch_buf* dst, size_t dst_first) try {
    if (!src || !dst) return fail(ALCH_E_INVALID, "null buffer");
    if (src->ring != dst->ring) return fail(ALCH_E_INVALID, "buffers belong to different rings");
    alch_ring* r = src->ring;
    BIND(r);
    if (src_index >= src->n_elems || !range_ok(dst_first, (size_t)r->L, dst->n_elems)) return fail(ALCH_E_INVALID, "element range out of bounds");
    const char* c = reinterpret_cast<const char*>(src->dptr) + src_index * elem_bytes(r);
    char* dig = reinterpret_cast<char*>(dst->dptr) + dst_first * elem_bytes(r);
    // every word of the source element is read by L lanes, one per digit: it must lie outside all L digits
    if (bytes_overlap(dig, (size_t)r->L * elem_bytes(r), c, elem_bytes(r)))
        return fail(ALCH_E_INVALID, "alch_buf_decompose_triv: the source element lies inside the L digits that are written");
    const size_t total = (size_t)r->L * elem_words(r);
    if (r->word == 4) hipLaunchKernelGGL((k_decompose_triv<u32>), dim3(ew_grid(total)), dim3(256), 0, r->stream, r->d32, (const u32*)c, (u32*)dig, r->balanced ? 1 : 0);
    else hipLaunchKernelGGL((k_decompose_triv<u64>), dim3(ew_grid(total)), dim3(256), 0, r->stream, r->d64, (const u64*)c, (u64*)dig, r->balanced ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return ALCH_OK;
} catch (...) { return abi_catch(); }

extern "C" int alch_hint_load(alch_ring* r, int gadget, const int64_t* host_crt, alch_hint** out) try {
    if (!r || !host_crt || !out) return fail(ALCH_E_INVALID, "null argument");
    if (gadget_width(gadget) < 0) return fail(ALCH_E_INVALID, "alch_hint_load: unknown gadget");
    const size_t elems = 2 * (size_t)gadget_digits(r, gadget);
    BIND(r);                                                          // held across the closing synchronisation: the scratch is read until then
    ScratchBuf s;
    int rc = scratch_get(r, elems, &s.b);
    if (rc != ALCH_OK) return rc;
    if ((rc = alch_buf_upload(s.b, 0, elems, host_crt)) != ALCH_OK) return rc;
    rc = hint_from_device(r, gadget, s.b->dptr, out);
    if (rc == ALCH_OK) HIP_TRY(hipStreamSynchronize(r->stream));
    return rc;
} catch (...) { return abi_catch(); }

extern "C" int alch_hint_from_buf(alch_ring* r, int gadget, const alch_buf* src, alch_hint** out) try {
    if (!r || !src || !out) return fail(ALCH_E_INVALID, "null argument");
    if (gadget_width(gadget) < 0) return fail(ALCH_E_INVALID, "alch_hint_from_buf: unknown gadget");
    if (src->ring != r || src->n_elems < 2 * (size_t)gadget_digits(r, gadget))
        return fail(ALCH_E_INVALID, "hint source needs 2 ring elements per gadget digit");
    return hint_from_device(r, gadget, src->dptr, out);
} catch (...) { return abi_catch(); }

extern "C" int alch_hint_free(alch_hint* h) try {
    if (!h) return ALCH_OK;
    (void)hipSetDevice(h->ring->device);
    (void)hipStreamSynchronize(h->ring->stream);
    (void)hipFree(h->dptr);
    delete h;
    return ALCH_OK;
} catch (...) { return abi_catch(); }

extern "C" int alch_ct_add_public(alch_buf* dst, const alch_buf* src, size_t batch, const uint64_t* s, const alch_buf* pub, size_t pub_index) try {
    if (!dst || !src || !pub) return fail(ALCH_E_INVALID, "null buffer");
    alch_ring* r = dst->ring;
    if (src->ring != r || pub->ring != r) return fail(ALCH_E_INVALID, "buffers belong to different rings");
    if (!r->has_crt) return fail(ALCH_E_UNSUPPORTED, "scalar products are implemented for rings with Montgomery constants (prime moduli) only");
    if (!pairs_ok(batch, dst->n_elems) || !pairs_ok(batch, src->n_elems) || pub_index >= pub->n_elems) return fail(ALCH_E_INVALID, "count out of bounds");
    if (batch == 0) return ALCH_OK;
    const char* pp = reinterpret_cast<const char*>(pub->dptr) + pub_index * elem_bytes(r);
    if (shifted_overlap(dst->dptr, 2 * batch * elem_bytes(r), src->dptr, 2 * batch * elem_bytes(r)))
        return fail(ALCH_E_INVALID, "alch_ct_add_public: dst overlaps src without starting where it starts");
    if (bytes_overlap(dst->dptr, 2 * batch * elem_bytes(r), pp, elem_bytes(r)))       // read by the lanes of every ciphertext
        return fail(ALCH_E_INVALID, "alch_ct_add_public: the public element lies inside the 2*batch elements of dst that are written");
    BIND(r);
    const size_t words = 2 * batch * elem_words(r);
    if (r->word == 4) {
        typedef u32 W;
        Scal<W> sm; scal_to_mont<W>(r, s, 1, sm);
        ALCH_LAUNCH_VW(k_scale_add_bcast, r, words, r->stream, r->d32, (W*)dst->dptr, (const W*)src->dptr, (const W*)pp, words, sm);
    } else {
        typedef u64 W;
        Scal<W> sm; scal_to_mont<W>(r, s, 1, sm);
        ALCH_LAUNCH_VW(k_scale_add_bcast, r, words, r->stream, r->d64, (W*)dst->dptr, (const W*)src->dptr, (const W*)pp, words, sm);
    }
    HIP_TRY(hipGetLastError());
    return ALCH_OK;
} catch (...) { return abi_catch(); }

// ------------------------------------------------------------------------------------------------------
// general index: l / lInv, mulG / divG on device buffers
// ------------------------------------------------------------------------------------------------------
// Runs one column operator (kernel_gen.hpp) on elements first, first + stride, ... (count of them) of `data`.
template <typename W>
static int do_columns(alch_ring* r, GenOp op, void* data, size_t first, size_t count, size_t stride, const alch_ring* on = nullptr,
                      const void* src = nullptr) {
    // src != null: out of place, src[e] -> data[e] (same element layout and stride); on != null: queue on that ring's stream (do_crt)
    if (count == 0) return ALCH_OK;
    GenCall<W> g{};
    g.src = reinterpret_cast<const W*>(src);
    g.op = op;
    g.ring = &dev_ring<W>(r);
    g.gen = &gen_dev<W>(r);
    g.stream = (on ? on : r)->stream;
    g.data = reinterpret_cast<W*>(data);
    g.elem_stride = stride;
    g.zdom = r->zdom;
    g.fail_flag = r->d_flag;
    for (size_t done = 0; done < count;) {
        const size_t now = std::min<size_t>(count - done, ((size_t)1 << 30) / (size_t)r->L);
        g.first_poly = first + done * stride;
        g.npoly = now * (size_t)r->L;
        if (int rc = launch(g, "general-index column")) return rc;
        done += now;
    }
    return ALCH_OK;
}

static int columns(alch_ring* r, GenOp op, void* data, size_t first, size_t count, size_t stride, const alch_ring* on = nullptr,
                   const void* src = nullptr) {
    return ALCH_BY_WORD(r, do_columns, r, op, data, first, count, stride, on, src);
}

// mulG (divide = false) or divG on elements [first, first + count) of a buffer, basis ALCH_BASIS_*.
// Returns ALCH_OK, ALCH_NOT_DIVISIBLE (Lol's Nothing; the data are then unspecified) or an error.
static int buf_mulg_divg(alch_buf* b, size_t first, size_t count, int basis, bool divide) {
    if (!b) return fail(ALCH_E_INVALID, "null buffer");
    if (!range_ok(first, count, b->n_elems)) return fail(ALCH_E_INVALID, "element range out of bounds");
    if (basis != ALCH_BASIS_POW && basis != ALCH_BASIS_DEC && basis != ALCH_BASIS_CRT) return fail(ALCH_E_INVALID, "unknown basis");
    alch_ring* r = b->ring;
    BIND(r);
    if (basis == ALCH_BASIS_CRT && !r->has_crt) return fail(ALCH_E_NO_CRT, "this ring has no CRT basis");
    if (!r->gen || r->gh.rad == 1 || count == 0) return ALCH_OK;      // g = 1: two-power index
    if (basis == ALCH_BASIS_CRT) {
        const size_t words = count * elem_words(r);
        char* base = reinterpret_cast<char*>(b->dptr) + first * elem_bytes(r);
        if (r->word == 4) {
            GTab<u32> gt{};
            for (int j = 0; j < r->L; ++j) gt.p[j] = divide ? r->g32.gcrt_inv[j] : r->g32.gcrt[j];
            hipLaunchKernelGGL((k_mul_table<u32>), dim3(ew_grid(words)), dim3(256), 0, r->stream, r->d32, (u32*)base, words, gt);
        } else {
            GTab<u64> gt{};
            for (int j = 0; j < r->L; ++j) gt.p[j] = divide ? r->g64.gcrt_inv[j] : r->g64.gcrt[j];
            hipLaunchKernelGGL((k_mul_table<u64>), dim3(ew_grid(words)), dim3(256), 0, r->stream, r->d64, (u64*)base, words, gt);
        }
        HIP_TRY(hipGetLastError());
        return ALCH_OK;
    }
    if (!divide) return columns(r, basis == ALCH_BASIS_POW ? GEN_MULG_POW : GEN_MULG_DEC, b->dptr, first, count, 1);
    HIP_TRY(hipMemsetAsync(r->d_flag, 0, sizeof(int), r->stream));
    int rc = columns(r, basis == ALCH_BASIS_POW ? GEN_DIVG_POW : GEN_DIVG_DEC, b->dptr, first, count, 1);
    if (rc != ALCH_OK) return rc;
    int flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, r->d_flag, sizeof(int), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return flag ? ALCH_NOT_DIVISIBLE : ALCH_OK;
}

extern "C" int alch_buf_mulg(alch_buf* b, size_t first, size_t count, int basis) try { return buf_mulg_divg(b, first, count, basis, false); } catch (...) { return abi_catch(); }
extern "C" int alch_buf_divg(alch_buf* b, size_t first, size_t count, int basis) try { return buf_mulg_divg(b, first, count, basis, true); } catch (...) { return abi_catch(); }

static int buf_l(alch_buf* b, size_t first, size_t count, bool inverse) {
    if (!b) return fail(ALCH_E_INVALID, "null buffer");
    if (!range_ok(first, count, b->n_elems)) return fail(ALCH_E_INVALID, "element range out of bounds");
    alch_ring* r = b->ring;
    BIND(r);
    if (!r->gen || r->gh.rad == 1) return ALCH_OK;                    // L = identity for a two-power index
    return columns(r, inverse ? GEN_LINV : GEN_L, b->dptr, first, count, 1);
}
extern "C" int alch_buf_l(alch_buf* b, size_t first, size_t count) try { return buf_l(b, first, count, false); } catch (...) { return abi_catch(); }
extern "C" int alch_buf_linv(alch_buf* b, size_t first, size_t count) try { return buf_l(b, first, count, true); } catch (...) { return abi_catch(); }

// ------------------------------------------------------------------------------------------------------
// device-resident Tensor values: what a `GT m r` holds when it stays on the GPU between Tensor calls
// ------------------------------------------------------------------------------------------------------
// E issues one Lol call per op (Crypto/Alchemy/Interpreter/Eval.hs:120-134) and Lol one Tensor call per basis change, so a
// ciphertext operation reaches this library as a chain of single-element calls.  With the host-buffer entry points every link
// of that chain crosses PCIe twice; with these the element stays in HBM and a link costs one kernel launch.
extern "C" int alch_ring_share_stream(alch_ring* r, alch_ring* with) try {
    if (!r || !with) return fail(ALCH_E_INVALID, "null ring");
    if (r->device != with->device) return fail(ALCH_E_INVALID, "alch_ring_share_stream: the rings live on different devices");
    if (r == with) return ALCH_OK;
    BIND(r);                                                          // one device, one lock: both rings' stream members are read under it
    if (r->stream == with->stream) return ALCH_OK;
    HIP_TRY(hipStreamSynchronize(r->stream));
    r->stream_owner = with->stream_owner;          // releases r's own stream (destroyed with its last user), keeps with's alive
    r->stream = with->stream;
    return ALCH_OK;
} catch (...) { return abi_catch(); }

extern "C" int alch_buf_copy(alch_buf* dst, size_t dst_first, const alch_buf* src, size_t src_first, size_t count) try {
    if (!dst || !src) return fail(ALCH_E_INVALID, "null buffer");
    if (dst->ring != src->ring) return fail(ALCH_E_INVALID, "buffers belong to different rings");
    if (!range_ok(dst_first, count, dst->n_elems) || !range_ok(src_first, count, src->n_elems)) return fail(ALCH_E_INVALID, "element range out of bounds");
    if (count == 0) return ALCH_OK;
    alch_ring* r = dst->ring;
    BIND(r);
    char* d = reinterpret_cast<char*>(dst->dptr) + dst_first * elem_bytes(r);
    const char* f = reinterpret_cast<const char*>(src->dptr) + src_first * elem_bytes(r);
    if (d == f) return ALCH_OK;
    if ((d < f ? f - d : d - f) < (ptrdiff_t)(count * elem_bytes(r))) return fail(ALCH_E_INVALID, "alch_buf_copy: overlapping ranges");
    HIP_TRY(hipMemcpyAsync(d, f, count * elem_bytes(r), hipMemcpyDeviceToDevice, r->stream));
    return ALCH_OK;
} catch (...) { return abi_catch(); }

// dst[dst_first + i] = op(src[src_first + i]), i < count.  Transforms and column operators read `src` and write `dst` in one
// kernel; the CRT-basis g products copy first.  dst and src may be the same range (in place).
extern "C" int alch_buf_tensor_op(alch_buf* dst, size_t dst_first, const alch_buf* src, size_t src_first, size_t count, int op) try {
    if (!dst || !src) return fail(ALCH_E_INVALID, "null buffer");
    if (dst->ring != src->ring) return fail(ALCH_E_INVALID, "buffers belong to different rings");
    if (!range_ok(dst_first, count, dst->n_elems) || !range_ok(src_first, count, src->n_elems)) return fail(ALCH_E_INVALID, "element range out of bounds");
    if (op < ALCH_T_CRT || op > ALCH_T_DIVG_CRT) return fail(ALCH_E_INVALID, "alch_buf_tensor_op: unknown op");
    alch_ring* r = dst->ring;
    BIND(r);
    const bool needs_crt = op == ALCH_T_CRT || op == ALCH_T_CRTINV || op == ALCH_T_MULG_CRT || op == ALCH_T_DIVG_CRT;
    if (needs_crt && !r->has_crt) return fail(ALCH_E_NO_CRT, "this ring has no CRT basis (created with alch_ring_create_nocrt)");
    if (count == 0) return ALCH_OK;
    char* d = reinterpret_cast<char*>(dst->dptr) + dst_first * elem_bytes(r);
    const char* f = reinterpret_cast<const char*>(src->dptr) + src_first * elem_bytes(r);
    const bool in_place = d == f;
    if (!in_place && (d < f ? f - d : d - f) < (ptrdiff_t)(count * elem_bytes(r))) return fail(ALCH_E_INVALID, "alch_buf_tensor_op: overlapping ranges");
    auto copy_first = [&]() -> int {
        if (!in_place) HIP_TRY(hipMemcpyAsync(d, f, count * elem_bytes(r), hipMemcpyDeviceToDevice, r->stream));
        return ALCH_OK;
    };
    int rc;
    if (op == ALCH_T_CRT || op == ALCH_T_CRTINV) {
        const bool inv = op == ALCH_T_CRTINV;
        if (in_place) return ALCH_BY_WORD(r, do_crt, r, d, 0, count, inv);
        return ALCH_BY_WORD(r, crt_into, r, d, {f}, count, inv);
    }
    const bool trivial = !r->gen || r->gh.rad == 1;                   // two-power index: g = 1, L = identity
    if (trivial) return copy_first();
    if (op == ALCH_T_MULG_CRT || op == ALCH_T_DIVG_CRT) {
        if ((rc = copy_first()) != ALCH_OK) return rc;
        alch_buf view{r, count, d};
        return buf_mulg_divg(&view, 0, count, ALCH_BASIS_CRT, op == ALCH_T_DIVG_CRT);
    }
    GenOp g = GEN_L;
    bool divide = false;
    switch (op) {
    case ALCH_T_L: g = GEN_L; break;
    case ALCH_T_LINV: g = GEN_LINV; break;
    case ALCH_T_MULG_POW: g = GEN_MULG_POW; break;
    case ALCH_T_MULG_DEC: g = GEN_MULG_DEC; break;
    case ALCH_T_DIVG_POW: g = GEN_DIVG_POW; divide = true; break;
    default: g = GEN_DIVG_DEC; divide = true; break;
    }
    if (divide) HIP_TRY(hipMemsetAsync(r->d_flag, 0, sizeof(int), r->stream));
    rc = columns(r, g, d, 0, count, 1, nullptr, in_place ? nullptr : f);
    if (rc != ALCH_OK || !divide) return rc;
    int flag = 0;                                                     // Lol's Maybe: the answer is needed now
    HIP_TRY(hipMemcpyAsync(&flag, r->d_flag, sizeof(int), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return flag ? ALCH_NOT_DIVISIBLE : ALCH_OK;
} catch (...) { return abi_catch(); }

extern "C" int alch_buf_mul_public(alch_buf* dst, const alch_buf* src, const alch_buf* pub, size_t pub_index, size_t count) try {
    if (!dst || !src || !pub) return fail(ALCH_E_INVALID, "null buffer");
    alch_ring* r = dst->ring;
    if (src->ring != r || pub->ring != r) return fail(ALCH_E_INVALID, "buffers belong to different rings");
    if (!r->has_crt) return fail(ALCH_E_NO_CRT, "this ring has no CRT basis");
    if (count > dst->n_elems || count > src->n_elems || pub_index >= pub->n_elems) return fail(ALCH_E_INVALID, "count out of bounds");
    const char* pp = reinterpret_cast<const char*>(pub->dptr) + pub_index * elem_bytes(r);
    if (count && shifted_overlap(dst->dptr, count * elem_bytes(r), src->dptr, count * elem_bytes(r)))
        return fail(ALCH_E_INVALID, "alch_buf_mul_public: dst overlaps src without starting where it starts");
    if (count && bytes_overlap(dst->dptr, count * elem_bytes(r), pp, elem_bytes(r)))  // read by the lanes of every element
        return fail(ALCH_E_INVALID, "alch_buf_mul_public: the public element lies inside the count elements of dst that are written");
    BIND(r);
    const size_t words = count * elem_words(r);
    if (r->word == 4) hipLaunchKernelGGL((k_mul_bcast<u32>), dim3(ew_grid(words)), dim3(256), 0, r->stream, r->d32, (u32*)dst->dptr, (const u32*)src->dptr, (const u32*)pp, words);
    else hipLaunchKernelGGL((k_mul_bcast<u64>), dim3(ew_grid(words)), dim3(256), 0, r->stream, r->d64, (u64*)dst->dptr, (const u64*)src->dptr, (const u64*)pp, words);
    HIP_TRY(hipGetLastError());
    return ALCH_OK;
} catch (...) { return abi_catch(); }

extern "C" int alch_buf_add_public(alch_buf* cts, const alch_buf* pub, size_t pub_index, size_t batch) try {
    if (!cts || !pub) return fail(ALCH_E_INVALID, "null buffer");
    alch_ring* r = cts->ring;
    if (pub->ring != r) return fail(ALCH_E_INVALID, "buffers belong to different rings");
    if (!pairs_ok(batch, cts->n_elems) || pub_index >= pub->n_elems) return fail(ALCH_E_INVALID, "count out of bounds");
    const char* pp = reinterpret_cast<const char*>(pub->dptr) + pub_index * elem_bytes(r);
    // only the c0 components (even elements) are written, but the ciphertext range is refused as a whole, c1 components included: one
    // rule for the three public-element entry points and for alch_buf_add_bcast
    if (batch && bytes_overlap(cts->dptr, 2 * batch * elem_bytes(r), pp, elem_bytes(r)))
        return fail(ALCH_E_INVALID, "alch_buf_add_public: the public element lies inside the 2*batch elements of cts");
    BIND(r);
    const size_t words = batch * elem_words(r);
    if (r->word == 4) hipLaunchKernelGGL((k_add_bcast<u32>), dim3(ew_grid(words)), dim3(256), 0, r->stream, r->d32, (u32*)cts->dptr, (const u32*)pp, batch);
    else hipLaunchKernelGGL((k_add_bcast<u64>), dim3(ew_grid(words)), dim3(256), 0, r->stream, r->d64, (u64*)cts->dptr, (const u64*)pp, batch);
    HIP_TRY(hipGetLastError());
    return ALCH_OK;
} catch (...) { return abi_catch(); }

// ------------------------------------------------------------------------------------------------------
// the hot path
// ------------------------------------------------------------------------------------------------------
// order work's stream after everything queued on other's stream (before), or hand back: other's stream after work's (!before)
static int ext_order(alch_ring* work, alch_ring* other, bool before) {
    if (work->stream == other->stream) return ALCH_OK;
    if (!work->ev_x) HIP_TRY(hipEventCreateWithFlags(&work->ev_x, hipEventDisableTiming));
    if (before) { HIP_TRY(hipEventRecord(work->ev_x, other->stream)); HIP_TRY(hipStreamWaitEvent(work->stream, work->ev_x, 0)); }
    else { HIP_TRY(hipEventRecord(work->ev_x, work->stream)); HIP_TRY(hipStreamWaitEvent(other->stream, work->ev_x, 0)); }
    return ALCH_OK;
}

// CRT image of g in Montgomery form, per limb (SymmSHE's (*) applies mulG); all-null where g = 1 (two-power index, radical 1)
template <typename W>
static GTab<W> g_table(alch_ring* r) {
    GTab<W> gt{};
    if (r->gen && r->gh.rad > 1) for (int j = 0; j < r->L; ++j) gt.p[j] = gen_dev<W>(r).gcrt[j];
    return gt;
}

// modSwitch up folded into a scalar: s times the `dup` leading moduli of r that the switch adds (inverse: divided by them), mod q_j
static u64 up_scalar(const alch_ring* r, int dup, int j, u64 s, bool inverse = false) {
    const u64 qj = r->q[j];
    u64 v = s % qj;
    for (int u = 0; u < dup; ++u) v = h_mulmod(v, inverse ? h_invmod(r->q[u] % qj, qj) : r->q[u] % qj, qj);
    return v;
}

// q_u^-1 mod q_(u+j) in Montgomery form, j = 1 .. L - u - 1: k_rescale_drop0's constants on the suffix ring that starts at limb u
template <typename W>
static Scal<W> drop0_inv_mont(const alch_ring* r, int u) {
    Scal<W> sm;
    for (int j = 0; j < MAXL; ++j) sm.v[j] = 0;
    for (int j = 1; u + j < r->L; ++j) {
        const u64 qj = r->q[u + j];
        sm.v[j] = (W)h_mulmod(h_powmod(r->q[u] % qj, qj - 2, qj), h_powmod(2, 8 * (u64)sizeof(W), qj), qj);
    }
    return sm;
}

// DevRing of the suffix ring that starts at limb u of r (device tables shared with the ring itself)
template <typename W>
static DevRing<W> suffix_view(const alch_ring* r, int u) {
    DevRing<W> d = dev_ring<W>(r);
    d.L = r->L - u;
    for (int j = 0; j + u < r->L; ++j) {
        d.mod[j] = d.mod[j + u]; d.ninv_m[j] = d.ninv_m[j + u]; d.w1ninv_m[j] = d.w1ninv_m[j + u];
        d.twf[j] = d.twf[j + u]; d.twi[j] = d.twi[j + u]; d.twp[j] = d.twp[j + u]; d.twpi[j] = d.twpi[j + u];
        d.tws[j] = d.tws[j + u]; d.twsi[j] = d.twsi[j + u];
    }
    return d;
}

// View of the last L - u limbs of a general-index ring (device tables shared with the ring itself).
template <typename W>
static void gen_suffix_view(alch_ring* r, int u, DevRing<W>& d, GenDev<W>& g) {
    d = dev_ring<W>(r);
    g = gen_dev<W>(r);
    d.L = r->L - u;
    for (int j = 0; j + u < r->L; ++j) {
        d.mod[j] = d.mod[j + u];
        g.tabf[j] = g.tabf[j + u]; g.tabi[j] = g.tabi[j + u]; g.iscale_m[j] = g.iscale_m[j + u];
        g.gcrt[j] = g.gcrt[j + u]; g.gcrt_inv[j] = g.gcrt_inv[j + u]; g.radinv_m[j] = g.radinv_m[j + u];
    }
}

// The fused general-index key switch (k_gen_tensor_inv + k_gen_ks, kernel_gen.hpp): TrivGad, 32-bit words, n <= 12288.
static bool gen_ks_fused(const alch_ring* r, const alch_hint* hint) {
    return r->gen && r->word == 4 && gadget_width(hint->gadget) == 0 && r->n <= (u32)(GEN_KS_T * GEN_KS_NPT) && r->opts.gen_fused;
}

template <typename W>
static void launch_hint_mac(alch_ring* r, hipStream_t stream, W* out, const W* digits, const W* hint, size_t nct, u32 D,
                            const W* diag = nullptr, u32 grp = 0, u32 hskip = 0, const u32* slot_e = nullptr, u32 n_d = 0,
                            bool pieces_ok = false) {
    if (slot_e && pieces_ok && !diag && r->n % Vec4<W>::LANES == 0) {
        const size_t pieces = (nct + 3) / 4 * (size_t)r->L * (r->n / Vec4<W>::LANES);
        hipLaunchKernelGGL((k_hint_mac_e<W, 4>), dim3(ew_grid(pieces)), dim3(256), 0, stream, dev_ring<W>(r), out, digits, hint, nct, D, grp, hskip, slot_e, n_d);
    } else if (r->n % Vec4<W>::LANES == 0) {
        const size_t pieces = (nct + 3) / 4 * (size_t)r->L * (r->n / Vec4<W>::LANES);
        hipLaunchKernelGGL((k_hint_mac_v<W, 4>), dim3(ew_grid(pieces)), dim3(256), 0, stream, dev_ring<W>(r), out, digits, hint, nct, D, diag, grp, hskip, slot_e, n_d);
    } else {
        hipLaunchKernelGGL((k_hint_mac<W>), dim3(ew_grid(nct * elem_words(r))), dim3(256), 0, stream, dev_ring<W>(r), out, digits, hint, nct, D, diag, grp, hskip, slot_e, n_d);
    }
}

// ---- the composed key switch: keySwitchQuadCirc hint (a * b) from the element-wise kernels and batched transforms -------------
// Element-wise tensor product, batched crtInv of c2, decompose, batched crt of the digits, hint inner product.  Serves
//   * BaseBGad 2 hints (PT2CT.hs:140; Tunnel.hs:24 / HomomRLWR.hs:46 pick that gadget): D = sum_i ceil(log2 q_i)
//     digits, each reduced into every limb and transformed -- D*L crt per ciphertext against L*(L-1) for TrivGad,
//     two orders of magnitude heavier by construction;
//   * TrivGad on rings too large for one LDS-resident transform (n = 2^16 / 2^15), where the fused kernels do
//     not exist and crt runs as k_crt_split;
//   * TrivGad on general-index rings.
// KsStage holds what every chunk of one call shares: which digit kernel serves (the only copy of that ladder's predicates), the
// scratch a ciphertext needs under them, and the operands that do not move with the chunk.
template <typename W>
struct KsStage {
    const alch_hint* hint;
    int dup;                    // leading limbs of r the operands lack: the modSwitch up of alch_ct_mul_full, folded in
    bool have_c2;               // c2 arrives on the powerful basis of r: no tensor product, no c2 scratch
    bool c2_both;               // with have_c2: the caller filled the stage's own layout -- c2 (Pow) at scratch, its CRT copy behind it, digits after
                                // both (alch_ct_key_switch_quad: the TrivGad forms below read the diagonal digits from the CRT copy)
    bool base2;                 // BaseBGad 2^gw
    u32 gw;                     // log2 of its base
    bool fused_digits;          // TrivGad: decompose + reduce in the digit transforms' loader; the diagonal digits are c2's CRT copy
    bool gen_fused;             // k_gen_tensor_inv + k_gen_ks
    bool no_digits;             // the one-kernel forms (k_ks_accum_split, k_gen_ks) keep no digits in HBM: only c2 in both bases
    bool compact;               // general index below the hint's ring: the limbs the first modSwitch adds are zero in c2, so c2, its crtInv and
                                // its digits are kept on the operands' L - dup limbs only (a fifth to a half of the digit transforms of PT2CT's products)
    u32 D;                      // gadget digits per ciphertext
    Scal<u32> first, kd;        // BaseBGad 2 layout
    size_t elems;               // scratch per ciphertext, in ring elements: c2 in both bases (unless it arrives ready) + digits (unless no_digits)
    Scal<W> sr2;                // the tensor product's scalar (times R^2)
    GTab<W> gt;
    W *c2, *c2crt, *dig;        // the stage's scratch, each for one chunk of ciphertexts: ks_stage_carve
};

template <typename W>
static KsStage<W> ks_stage_plan(alch_ring* r, const alch_hint* hint, int dup, bool have_c2) {
    KsStage<W> s{};
    s.hint = hint; s.dup = dup; s.have_c2 = have_c2;
    s.gw = (u32)gadget_width(hint->gadget);
    s.base2 = s.gw > 0;
    s.D = s.base2 ? (u32)base2_layout(r, s.first, s.kd, s.gw) : (u32)r->L;
    s.fused_digits = !s.base2 && (split_ring(r) || r->gen);
    s.gen_fused = !have_c2 && gen_ks_fused(r, hint);
    s.no_digits = s.fused_digits && ((!r->gen && r->opts.split_fused) || s.gen_fused);
    s.compact = r->gen && dup > 0;
    s.elems = (have_c2 ? 0 : 2) + (s.no_digits ? 0 : s.D);
    if (!have_c2) s.gt = g_table<W>(r);
    return s;
}
// The stage's regions, next in the caller's arena: c2 | c2crt | dig (a ready c2 that is not the stage's own, BaseBGad 2 only: dig alone).
template <typename W>
static void ks_stage_carve(KsStage<W>& s, Carve& cv, size_t eb) {
    const size_t c2_b = (s.have_c2 && !s.c2_both) ? 0 : eb;
    s.c2 = reinterpret_cast<W*>(cv.take(c2_b));
    s.c2crt = reinterpret_cast<W*>(cv.take(c2_b));                // CRT-basis copy of c2 (diagonal digits, split rings)
    s.dig = reinterpret_cast<W*>(cv.take(s.no_digits ? 0 : s.D * eb));
}

// The stage for `now` ciphertexts, at most the chunk it was carved for: out [now][2][L][n] = (c0, c1) of a * b + switch(hint, c2).  a, b: the operands on the last
// L - s.dup limbs of r; or, for s.have_c2, c2pow: `now` elements of r, and out already holds (c0, c1).
template <typename W>
static int ks_stage(alch_ring* r, const KsStage<W>& s, const W* a, const W* b, const W* c2pow, W* out, size_t now) {
    const int L = r->L, Ls = L - s.dup;
    const W* hint = reinterpret_cast<const W*>(s.hint->dptr);
    W *dig = s.dig, *diag = s.fused_digits ? s.c2crt : nullptr;
    NttCall<W> nc{};
    nc.ring = &dev_ring<W>(r); nc.stream = r->stream; nc.balanced = r->balanced;
    GenCall<W> gc{};
    gc.ring = &dev_ring<W>(r); gc.gen = &gen_dev<W>(r); gc.stream = r->stream; gc.balanced = r->balanced;
    int rc;
    if (!s.have_c2) {
        W* c2 = s.c2;
        if constexpr (sizeof(W) == 4) {
            if (s.gen_fused) {                                    // two fused launches: tensor + crtInv, digit transforms + hint products
                GenKsArgs<u32> A{};
                A.a = a; A.b = b; A.c2pow = c2; A.hint = hint; A.out = out;
                A.sr2 = s.sr2; A.dup = s.dup; A.balanced = r->balanced ? 1 : 0; A.use_g = r->gh.rad > 1 ? 1 : 0;
                const hipError_t e = gen_ks_dispatch(r->d32, r->g32, A, now, r->stream);
                return e == hipSuccess ? ALCH_OK : fail(ALCH_E_HIP, std::string("general-index fused key switch launch: ") + hipGetErrorString(e));
            }
        }
        // (*) and modSwitch up
        ALCH_LAUNCH_VW(k_tensor_ew, r, now * elem_words(r), r->stream, dev_ring<W>(r), a, b, out, c2, now, s.sr2, s.dup,
                       diag, s.gt, s.compact ? 1 : 0);
        HIP_TRY(hipGetLastError());
        if (s.compact) {
            DevRing<W> dv; GenDev<W> gv;
            gen_suffix_view<W>(r, s.dup, dv, gv);
            GenCall<W> g{};
            g.op = GEN_CRTINV; g.ring = &dv; g.gen = &gv; g.stream = r->stream;
            g.data = c2; g.first_poly = 0; g.npoly = now * (size_t)Ls;
            if ((rc = launch(g, "general-index crtInv")) != ALCH_OK) return rc;
        } else if ((rc = do_crt<W>(r, c2, 0, now, true)) != ALCH_OK) return rc;
        c2pow = c2;
    }
    nc.src = gc.src = c2pow;
    if (s.fused_digits && r->gen) {                               // general index: decompose + reduce in the pass engine's loader
        gc.op = GEN_CRT_DIGITS;
        gc.data = dig;
        gc.npoly = now * (size_t)Ls * (size_t)L;
        if (s.compact) { gc.src_limbs = Ls; gc.src_first = s.dup; }
        if ((rc = launch(gc, "general-index crt_digits")) != ALCH_OK) return rc;
    } else if (s.fused_digits && r->opts.split_fused) {           // split rings: digit transforms + hint products in one kernel (k_ks_accum_split)
        nc.op = OP_KS_SPLIT;
        nc.a = diag; nc.hint = hint; nc.out = out; nc.nct = now; nc.dup = s.dup;
        return launch(r, nc, "ks_accum_split");
    } else if (s.fused_digits) {                                  // decompose + reduce fused into the digit transforms (k_crt_split_digits)
        nc.op = OP_CRT_DIGITS;
        nc.data = dig;
        nc.npoly = now * (size_t)L * (size_t)L;
        if ((rc = launch(r, nc, "crt_digits")) != ALCH_OK) return rc;
    } else if (s.base2 && !split_ring(r) && !r->gen) {            // BaseBGad: digits computed in the transforms' loader
        nc.op = OP_CRT_BASE2;
        nc.data = dig;
        nc.npoly = now * (size_t)s.D * (size_t)L;
        nc.b2_first = s.first; nc.b2_kd = s.kd; nc.b2_D = s.D; nc.b2_w = s.gw;
        if ((rc = launch(r, nc, "crt_base2")) != ALCH_OK) return rc;
    } else {
        for (size_t y0 = 0; y0 < now; y0 += 32768) {             // grid.y is 16-bit
            const unsigned ny = (unsigned)std::min<size_t>(32768, now - y0);
            const W* src = c2pow + y0 * elem_words(r);
            W* dst = dig + y0 * s.D * elem_words(r);
            if (s.base2)
                launch_decompose_baseb<W>(r, r->stream, dev_ring<W>(r), ny, src, dst, s.first, s.kd, s.D, s.gw);
            else
                hipLaunchKernelGGL((k_decompose_triv<W>), dim3(ew_grid((size_t)L * elem_words(r)), ny), dim3(256), 0,
                                   r->stream, dev_ring<W>(r), src, dst, r->balanced ? 1 : 0);
            HIP_TRY(hipGetLastError());
        }
        if ((rc = do_crt<W>(r, dig, 0, now * s.D, false)) != ALCH_OK) return rc;
    }
    if (s.compact) launch_hint_mac<W>(r, r->stream, out, dig, hint, now, (u32)Ls, diag, (u32)Ls, (u32)s.dup);
    else launch_hint_mac<W>(r, r->stream, out, dig, hint, now, s.D, diag);
    HIP_TRY(hipGetLastError());
    return ALCH_OK;
}

// The composed key switch of alch_ct_mul_relin, in chunks of at most scratch_mib of scratch (~1 GiB).  With c2pow, keySwitchQuadCirc's
// second half for BaseBGad 2 from a c2 that is already on the powerful basis of the hint's ring (mul_full_base2_down):
// out (c0, c1 on the CRT basis) += sum_d crt(digit_d(c2)) * hint_d.
template <typename W>
static int do_mul_relin_unfused(alch_ring* r, const alch_hint* hint, const void* a, const void* b, void* out, size_t batch,
                                const uint64_t* s_pre, const void* c2pow = nullptr) {
    KsStage<W> s = ks_stage_plan<W>(r, hint, 0, c2pow != nullptr);
    const size_t per_ct = s.elems * elem_bytes(r);
    const size_t chunk = scratch_chunk(r->scratch_mib << 20, batch, per_ct);
    int rc = r->ws_digits.reserve(chunk * per_ct);
    if (rc != ALCH_OK) return rc;
    Carve cv(r->ws_digits.p, chunk);
    ks_stage_carve(s, cv, elem_bytes(r));
    if (!cv.matches(per_ct)) return fail(ALCH_E_INTERNAL, "do_mul_relin_unfused: the scratch carve differs from the bytes reserved per ciphertext");
    if (!c2pow) scal_to_mont<W>(r, s_pre, 2, s.sr2);
    const size_t ew = elem_words(r);
    for (size_t done = 0; done < batch; done += chunk) {
        const size_t now = std::min(chunk, batch - done);
        const W* pa = c2pow ? nullptr : reinterpret_cast<const W*>(a) + done * 2 * ew;
        const W* pb = c2pow ? nullptr : reinterpret_cast<const W*>(b) + done * 2 * ew;
        const W* pc = c2pow ? reinterpret_cast<const W*>(c2pow) + done * ew : nullptr;
        if ((rc = ks_stage<W>(r, s, pa, pb, pc, reinterpret_cast<W*>(out) + done * 2 * ew, now)) != ALCH_OK) return rc;
    }
    return ALCH_OK;
}

template <typename W>
static int do_mul_relin(alch_ring* r, const alch_hint* hint, const void* a, const void* b, void* out, size_t batch,
                        const uint64_t* s_pre) {
    typedef typename Signed<W>::type SW;
    // The batch runs as chunks of (tensor_intt, ks_accum) launch pairs.  A chunk's digits (chunk * L * n
    // signed words) are written by the first kernel and read 2(L-1) times by the second, so the chunk is kept
    // small enough for them to stay in the 256 MiB Infinity Cache; to keep the GPU full across the kernel
    // boundaries of such small launches, even and odd chunks run as two independent pipelines on two streams
    // (each with its own digit scratch), so one pipeline's tail overlaps the other's head.
    const size_t chunk = fused_chunk(r->chunk, 2 * elem_bytes(r), batch);        // 32-bit byte offsets per array, groups of 8
    const size_t dig_bytes = chunk * elem_words(r) * sizeof(SW);
    const int ns = r->one_stream ? 1 : r->nstreams;
    int rc = r->ws_digits.reserve((size_t)std::max(2, ns) * dig_bytes);
    if (rc != ALCH_OK) return rc;
    for (int e = 0; e + 2 < ns; ++e) {
        if (!r->xs[e]) HIP_TRY(hipStreamCreateWithFlags(&r->xs[e], hipStreamNonBlocking));
        if (!r->ev_xs[e]) HIP_TRY(hipEventCreateWithFlags(&r->ev_xs[e], hipEventDisableTiming));
    }
    hipStream_t lanes[4] = {r->stream, r->aux, r->xs[0], r->xs[1]};
    NttCall<W> c{};
    c.ring = &dev_ring<W>(r);
    c.hint = reinterpret_cast<const W*>(hint->dptr);
    c.balanced = r->balanced;
    c.opts = r->opts;
    c.q30 = r->q30 && r->opts.q30;
    c.partials = true;                              // read by ALCH_A_PARTIALS builds only (kernel_tensor_split.hpp)
    scal_to_mont<W>(r, s_pre, 2, c.spre_r2);
    const size_t ct_words = 2 * elem_words(r);
    const bool two = batch > chunk && !r->one_stream;
    if (two) {
        HIP_TRY(hipEventRecord(r->ev_fork, r->stream));
        for (int e = 1; e < ns; ++e) HIP_TRY(hipStreamWaitEvent(lanes[e], r->ev_fork, 0));
    }
    size_t idx = 0;
    if (two && r->pipe) {
        // Anti-phase pipeline: every tensor kernel on the aux stream, every key-switch kernel on the ring's stream, the tensor
        // kernel of chunk k+1 released as soon as chunk k-1's key switch has freed its digit scratch -- it shares the CUs with
        // chunk k's key switch (a latency-bound kernel next to a VALU-bound one) instead of with another tensor kernel.
        for (int e = 0; e < 2; ++e) {
            if (!r->ev_pa[e]) HIP_TRY(hipEventCreateWithFlags(&r->ev_pa[e], hipEventDisableTiming));
            if (!r->ev_pb[e]) HIP_TRY(hipEventCreateWithFlags(&r->ev_pb[e], hipEventDisableTiming));
        }
        // the tensor kernels run on the aux stream whatever `nstreams` says: order it behind everything queued on the ring's stream
        // (the producers of a and b, and the previous call's key-switch kernels, which still read the digit scratch)
        if (ns < 2) HIP_TRY(hipStreamWaitEvent(r->aux, r->ev_fork, 0));
        for (size_t done = 0; done < batch; done += chunk, ++idx) {
            const size_t now = std::min(chunk, batch - done);
            const int par = (int)(idx & 1);
            c.digits = reinterpret_cast<char*>(r->ws_digits.p) + (par ? dig_bytes : 0);
            c.a = reinterpret_cast<const W*>(a) + done * ct_words;
            c.b = reinterpret_cast<const W*>(b) + done * ct_words;
            c.out = reinterpret_cast<W*>(out) + done * ct_words;
            c.nct = now;
            if (idx >= 2) HIP_TRY(hipStreamWaitEvent(r->aux, r->ev_pb[par], 0));
            c.stream = r->aux;
            c.op = OP_TENSOR_INTT;
            if ((rc = launch(r, c, "tensor_intt")) != ALCH_OK) return rc;
            HIP_TRY(hipEventRecord(r->ev_pa[par], r->aux));
            HIP_TRY(hipStreamWaitEvent(r->stream, r->ev_pa[par], 0));
            c.stream = r->stream;
            c.op = OP_KS_ACCUM;
            if ((rc = launch(r, c, "ks_accum")) != ALCH_OK) return rc;
            HIP_TRY(hipEventRecord(r->ev_pb[par], r->stream));
        }
        return ALCH_OK;                                    // the last key switch is on the ring's stream, behind every tensor kernel
    }
    for (size_t done = 0; done < batch; done += chunk, ++idx) {
        const size_t now = std::min(chunk, batch - done);
        const int lane = two ? (int)(idx % (size_t)ns) : 0;
        c.stream = lanes[lane];
        c.digits = reinterpret_cast<char*>(r->ws_digits.p) + (size_t)lane * dig_bytes;
        c.a = reinterpret_cast<const W*>(a) + done * ct_words;
        c.b = reinterpret_cast<const W*>(b) + done * ct_words;
        c.out = reinterpret_cast<W*>(out) + done * ct_words;
        c.nct = now;
        c.op = OP_TENSOR_INTT;
        if ((rc = launch(r, c, "tensor_intt")) != ALCH_OK) return rc;
        c.op = OP_KS_ACCUM;
        if ((rc = launch(r, c, "ks_accum")) != ALCH_OK) return rc;
    }
    if (two) {
        HIP_TRY(hipEventRecord(r->ev_join, r->aux));
        HIP_TRY(hipStreamWaitEvent(r->stream, r->ev_join, 0));
        for (int e = 2; e < ns; ++e) {
            HIP_TRY(hipEventRecord(r->ev_xs[e - 2], lanes[e]));
            HIP_TRY(hipStreamWaitEvent(r->stream, r->ev_xs[e - 2], 0));
        }
    }
    return ALCH_OK;
}

extern "C" int alch_ct_mul_relin(alch_ring* r, const alch_hint* hint, const alch_buf* a, const alch_buf* b, alch_buf* out,
                                 size_t batch, const uint64_t* s_pre, unsigned flags) try {
    if (!r || !hint || !a || !b || !out) return fail(ALCH_E_INVALID, "null argument");
    if (!r->has_crt) return fail(ALCH_E_NO_CRT, "this ring has no CRT basis");
    if (hint->ring != r || a->ring != r || b->ring != r || out->ring != r) return fail(ALCH_E_INVALID, "handles belong to different rings");
    if (batch == 0) return ALCH_OK;
    BIND(r);
    if (!pairs_ok(batch, a->n_elems) || !pairs_ok(batch, b->n_elems) || !pairs_ok(batch, out->n_elems))
        return fail(ALCH_E_INVALID, "buffers must hold 2*batch ring elements");
    // by bytes, not by handle: a view of an operand is another handle over the same words, and the fused kernels read the operands
    // chunk by chunk while earlier chunks write out
    if (bytes_overlap(out->dptr, 2 * batch * elem_bytes(r), a->dptr, 2 * batch * elem_bytes(r)) ||
        bytes_overlap(out->dptr, 2 * batch * elem_bytes(r), b->dptr, 2 * batch * elem_bytes(r)))
        return fail(ALCH_E_INVALID, "alch_ct_mul_relin: out must not alias an input");
    const void* pa = a->dptr;
    const void* pb = b->dptr;
    int rc;
    if (flags & ALCH_POW_IN) {
        const size_t bytes = 2 * batch * elem_bytes(r);
        if ((rc = r->ws_in.reserve(2 * bytes)) != ALCH_OK) return rc;
        pa = r->ws_in.p;
        pb = reinterpret_cast<char*>(r->ws_in.p) + bytes;
        if ((rc = ALCH_BY_WORD(r, crt_into, r, r->ws_in.p, {a->dptr, b->dptr}, 2 * batch, false)) != ALCH_OK) return rc;
    }
    // split rings (a limb-polynomial is twice an LDS-resident transform), TrivGad: the same two-launch structure as the LDS-resident sizes
    // since round 3 (k_tensor_crtinv_split + k_ks_accum_split<FROM_OPS>); option split_fused < 2 keeps the composed forms
    const bool split_two = split_ring(r) && !r->gen && gadget_width(hint->gadget) == 0 && r->opts.split_fused >= 2;
    if (!split_two && (gadget_width(hint->gadget) > 0 || split_ring(r) || r->gen))
        rc = ALCH_BY_WORD(r, do_mul_relin_unfused, r, hint, pa, pb, out->dptr, batch, s_pre);
    else
        rc = ALCH_BY_WORD(r, do_mul_relin, r, hint, pa, pb, out->dptr, batch, s_pre);
    if (rc != ALCH_OK) return rc;
    if (flags & ALCH_POW_OUT) return buf_crt(out, 0, 2 * batch, true);
    return ALCH_OK;
} catch (...) { return abi_catch(); }

// ---- mul_ one SHE operation at a time (within ABI 1.8; a host probes for the symbols): (*) and keySwitchQuadCirc on their own -----
// PT2CT emits modSwitch_ . keySwitchQuad_ hint . modSwitch_ $ x *: y as four object-language operations (PT2CT.hs:160-177) and the
// ErrorRateWriter logs a rate after each; these entry points let the quadratic ciphertext exist in a caller's buffer, elements
// (3b, 3b+1, 3b+2) = (c0, c1, c2).  They are the inspection path: alch_ct_mul_relin / alch_ct_mul_full stay the fast one.
template <typename W>
static int do_ct_mul(alch_ring* r, const void* a, const void* b, void* out, size_t batch, const uint64_t* s_pre, unsigned flags) {
    Scal<W> sr2;
    scal_to_mont<W>(r, s_pre, 2, sr2);
    const GTab<W> gt = g_table<W>(r);
    const size_t eb = elem_bytes(r), ew = elem_words(r);
    const bool pow_in = (flags & ALCH_POW_IN) != 0;
    size_t chunk = batch;
    int rc;
    if (pow_in) {                                          // CRT copies of one chunk's operands: 2 + 2 elements per ciphertext
        chunk = scratch_chunk(r->scratch_mib << 20, batch, 4 * eb);
        if ((rc = r->ws_in.reserve(chunk * 4 * eb)) != ALCH_OK) return rc;
    }
    for (size_t done = 0; done < batch; done += chunk) {
        const size_t now = std::min(chunk, batch - done);
        const W* pa = reinterpret_cast<const W*>(a) + done * 2 * ew;
        const W* pb = reinterpret_cast<const W*>(b) + done * 2 * ew;
        if (pow_in) {                                      // both operands contiguous: on a split ring, one transform launch
            if ((rc = crt_into<W>(r, r->ws_in.p, {pa, pb}, 2 * now, false)) != ALCH_OK) return rc;
            pa = reinterpret_cast<const W*>(r->ws_in.p);
            pb = pa + now * 2 * ew;
        }
        ALCH_LAUNCH_VW(k_ct_tensor3, r, now * ew, r->stream, dev_ring<W>(r), pa, pb, reinterpret_cast<W*>(out) + done * 3 * ew, now, sr2, gt);
        HIP_TRY(hipGetLastError());
        if ((flags & ALCH_POW_OUT) && (rc = do_crt<W>(r, out, 3 * done, 3 * now, true)) != ALCH_OK) return rc;
    }
    return ALCH_OK;
}

extern "C" int alch_ct_mul(alch_ring* r, const alch_buf* a, const alch_buf* b, alch_buf* out, size_t batch, const uint64_t* s_pre,
                           unsigned flags) try {
    if (!r || !a || !b || !out) return fail(ALCH_E_INVALID, "alch_ct_mul: null argument");
    if (a->ring != r || b->ring != r || out->ring != r) return fail(ALCH_E_INVALID, "alch_ct_mul: handles belong to different rings");
    if (!pairs_ok(batch, a->n_elems) || !pairs_ok(batch, b->n_elems) || batch > out->n_elems / 3)
        return fail(ALCH_E_INVALID, "alch_ct_mul: operands must hold 2*batch ring elements, out 3*batch");
    if (flags & ~(unsigned)(ALCH_POW_IN | ALCH_POW_OUT)) return fail(ALCH_E_INVALID, "alch_ct_mul: unknown flag");
    if (out == a || out == b || bytes_overlap(out->dptr, 3 * batch * elem_bytes(r), a->dptr, 2 * batch * elem_bytes(r)) ||
        bytes_overlap(out->dptr, 3 * batch * elem_bytes(r), b->dptr, 2 * batch * elem_bytes(r)))
        return fail(ALCH_E_INVALID, "alch_ct_mul: out must not alias an input");
    if (!r->has_crt) return fail(ALCH_E_NO_CRT, "alch_ct_mul: this ring has no CRT basis");
    if (batch == 0) return ALCH_OK;
    BIND(r);
    return ALCH_BY_WORD(r, do_ct_mul, r, a->dptr, b->dptr, out->dptr, batch, s_pre, flags);
} catch (...) { return abi_catch(); }

// ---- SymmSHE (+), (-), negate on resident batches, operands unaligned (within ABI 1.8; a host probes for the symbol) -------------------
// add_ = pureE (+) and neg_ = pureE negate (Eval.hs:59-60, PT2CT.hs:117-118).  SymmSHE's (+) owes its operands an alignment -- the
// g-power k, the Z_p scalar l, the MSD / LSD encoding, the degree -- and all of it is per-limb scalars and powers of the CRT image
// of g: one element-wise pass (k_ct_add), the metadata rule on the host (alchemy_amd/ctadd.py: align).
// The pack width follows ALCH_LAUNCH_VW's rule (that macro names kernels of two template parameters; this one has four).
template <typename W, int DA, int DB>
static int launch_ct_add(alch_ring* r, const W* a, const W* b, W* out, size_t nct, const Scal<W>& sa, const Scal<W>& sb,
                         const GTab<W>& gt, u32 ga, u32 gb, u32 scaled) {
    constexpr int VL = Vec4<W>::LANES;
    const size_t items = nct * elem_words(r);
    if (r->n % VL == 0)
        hipLaunchKernelGGL((k_ct_add<W, VL, DA, DB>), dim3(ew_grid(items / VL)), dim3(256), 0, r->stream, dev_ring<W>(r), a, b, out, nct,
                           sa, sb, gt, ga, gb, scaled);
    else
        hipLaunchKernelGGL((k_ct_add<W, 1, DA, DB>), dim3(ew_grid(items)), dim3(256), 0, r->stream, dev_ring<W>(r), a, b, out, nct,
                           sa, sb, gt, ga, gb, scaled);
    HIP_TRY(hipGetLastError());
    return ALCH_OK;
}

template <typename W>
static int do_ct_add(alch_ring* r, void* out, size_t batch, const void* a, int deg_a, const uint64_t* s_a, unsigned g_a,
                     const void* b, int deg_b, const uint64_t* s_b, unsigned g_b, bool pow_basis) {
    // deg_b = 0: no second operand
    Scal<W> sa, sb;
    scal_to_mont<W>(r, s_a, 1, sa);
    scal_to_mont<W>(r, s_b, 1, sb);
    const u32 scaled = (s_a ? 1u : 0u) | (s_b ? 2u : 0u);
    const bool has_g = r->gen && r->gh.rad > 1;                        // otherwise g = 1 and its powers are the identity
    if (!has_g) g_a = g_b = 0;
    const size_t eb = elem_bytes(r), ew = elem_words(r);
    const size_t ea = (size_t)deg_a + 1, ebb = (size_t)deg_b + 1, eo = (size_t)std::max(deg_a, deg_b) + 1;
    // Pow basis, general index: g is no pointwise factor there.  The operand that needs it goes through the batched mulG column
    // operator into the ring's scratch, chunk by chunk, and the pass reads it from there with no g-power left.
    const bool col_a = pow_basis && g_a, col_b = pow_basis && deg_b && g_b;
    size_t chunk = batch;
    if (col_a || col_b) {
        const size_t per_ct = ((col_a ? ea : 0) + (col_b ? ebb : 0)) * eb;
        chunk = scratch_chunk(r->scratch_mib << 20, batch, per_ct);
        if (int rc = r->ws_in.reserve(chunk * per_ct)) return rc;
    }
    const GTab<W> gt = pow_basis ? GTab<W>{} : g_table<W>(r);
    const u32 ka = pow_basis ? 0u : g_a, kb = pow_basis ? 0u : g_b;
    for (size_t done = 0; done < batch; done += chunk) {
        const size_t now = std::min(chunk, batch - done);
        const W* pa = reinterpret_cast<const W*>(a) + done * ea * ew;
        const W* pb = deg_b ? reinterpret_cast<const W*>(b) + done * ebb * ew : nullptr;
        char *wa = reinterpret_cast<char*>(r->ws_in.p), *wb = wa + (col_a ? now * ea * eb : 0);    // this chunk's operands, back to back
        if (col_a) {
            for (unsigned t = 0; t < g_a; ++t)
                if (int rc = do_columns<W>(r, GEN_MULG_POW, wa, 0, now * ea, 1, nullptr, t == 0 ? pa : nullptr)) return rc;
            pa = reinterpret_cast<const W*>(wa);
        }
        if (col_b) {
            for (unsigned t = 0; t < g_b; ++t)
                if (int rc = do_columns<W>(r, GEN_MULG_POW, wb, 0, now * ebb, 1, nullptr, t == 0 ? pb : nullptr)) return rc;
            pb = reinterpret_cast<const W*>(wb);
        }
        W* po = reinterpret_cast<W*>(out) + done * eo * ew;
        int rc;
        switch (deg_a * 3 + deg_b) {
        case 3: rc = launch_ct_add<W, 1, 0>(r, pa, pb, po, now, sa, sb, gt, ka, kb, scaled); break;
        case 4: rc = launch_ct_add<W, 1, 1>(r, pa, pb, po, now, sa, sb, gt, ka, kb, scaled); break;
        case 5: rc = launch_ct_add<W, 1, 2>(r, pa, pb, po, now, sa, sb, gt, ka, kb, scaled); break;
        case 6: rc = launch_ct_add<W, 2, 0>(r, pa, pb, po, now, sa, sb, gt, ka, kb, scaled); break;
        case 7: rc = launch_ct_add<W, 2, 1>(r, pa, pb, po, now, sa, sb, gt, ka, kb, scaled); break;
        default: rc = launch_ct_add<W, 2, 2>(r, pa, pb, po, now, sa, sb, gt, ka, kb, scaled); break;
        }
        if (rc != ALCH_OK) return rc;
    }
    return ALCH_OK;
}

extern "C" int alch_ct_add(alch_buf* out, size_t batch, const alch_buf* a, int deg_a, const uint64_t* s_a, unsigned g_a,
                           const alch_buf* b, int deg_b, const uint64_t* s_b, unsigned g_b, unsigned flags) try {
    if (!out || !a) return fail(ALCH_E_INVALID, "alch_ct_add: null buffer");
    alch_ring* r = out->ring;
    if (a->ring != r || (b && b->ring != r)) return fail(ALCH_E_INVALID, "alch_ct_add: buffers belong to different rings");
    if (!b) { deg_b = 0; s_b = nullptr; g_b = 0; }                     // the unary form ignores them
    if ((deg_a != 1 && deg_a != 2) || (b && deg_b != 1 && deg_b != 2)) return fail(ALCH_E_INVALID, "alch_ct_add: degree must be 1 or 2");
    if (flags & ~(unsigned)(ALCH_POW_IN | ALCH_POW_OUT)) return fail(ALCH_E_INVALID, "alch_ct_add: unknown flag");
    if (g_a > 16 || g_b > 16) return fail(ALCH_E_INVALID, "alch_ct_add: a g-power above 16");
    const size_t ea = (size_t)deg_a + 1, ebb = (size_t)deg_b + 1, eo = std::max(ea, ebb);
    if (batch > a->n_elems / ea || (b && batch > b->n_elems / ebb) || batch > out->n_elems / eo)
        return fail(ALCH_E_INVALID, "alch_ct_add: a buffer holds fewer than (degree + 1) * batch ring elements");
    // out may BE an operand of the result's degree (every word is read and written by one lane); any other overlap is refused
    const size_t eby = elem_bytes(r);
    auto alias_ok = [&](const alch_buf* x, size_t ex) {
        if (out->dptr == x->dptr) return ex == eo;
        return !bytes_overlap(out->dptr, eo * batch * eby, x->dptr, ex * batch * eby);
    };
    if (!alias_ok(a, ea) || (b && !alias_ok(b, ebb)))
        return fail(ALCH_E_INVALID, "alch_ct_add: out overlaps an operand without being that operand at the result's degree");
    const bool pow_basis = (flags & ALCH_POW_IN) != 0;
    if (pow_basis != ((flags & ALCH_POW_OUT) != 0))
        return fail(ALCH_E_UNSUPPORTED, "alch_ct_add: one basis in and out (0 or ALCH_POW_IN | ALCH_POW_OUT); alch_buf_crt / alch_buf_crtinv change it");
    if (!r->has_crt) {
        if (!pow_basis && (g_a || g_b)) return fail(ALCH_E_NO_CRT, "alch_ct_add: a g-power on the CRT basis of a ring that has none");
        return fail(ALCH_E_UNSUPPORTED, "scalar products are implemented for rings with Montgomery constants (prime moduli) only");
    }
    if (batch == 0) return ALCH_OK;
    BIND(r);
    return ALCH_BY_WORD(r, do_ct_add, r, out->dptr, batch, a->dptr, deg_a, s_a, g_a, b ? b->dptr : nullptr, deg_b, s_b, g_b, pow_basis);
} catch (...) { return abi_catch(); }

// keySwitchQuadCirc from a resident quadratic ciphertext, through the composed stage (ks_stage with a ready c2).  Per chunk:
// k_ct_split3 scales and gathers (c0, c1) into out and c2 into the stage's scratch (twice for the forms that read the diagonal digits
// from a CRT copy: the input is in the CRT basis, so that copy costs a store), crtInv of c2 in place, then the stage's ladder.
template <typename W>
static int do_key_switch_quad(alch_ring* r, const alch_hint* hint, const void* in, void* out, size_t batch, const uint64_t* s_pre,
                              unsigned flags) {
    KsStage<W> s = ks_stage_plan<W>(r, hint, 0, true);
    s.c2_both = true;
    const size_t eb = elem_bytes(r), ew = elem_words(r);
    const bool pow_in = (flags & ALCH_POW_IN) != 0;
    // scratch per ciphertext: c2 in both bases + the stage's digits (+ the CRT copy of a Pow-basis input)
    const size_t stage_elems = 2 + s.elems;
    const size_t per_ct = (stage_elems + (pow_in ? 3 : 0)) * eb;
    const size_t chunk = scratch_chunk(r->scratch_mib << 20, batch, per_ct);
    int rc = r->ws_digits.reserve(chunk * per_ct);
    if (rc != ALCH_OK) return rc;
    Carve cv(r->ws_digits.p, chunk);
    ks_stage_carve(s, cv, eb);
    char* win = cv.take(pow_in ? 3 * eb : 0);
    if (!cv.matches(per_ct)) return fail(ALCH_E_INTERNAL, "do_key_switch_quad: the scratch carve differs from the bytes reserved per ciphertext");
    W *c2pow = s.c2, *c2crt = s.fused_digits ? s.c2crt : nullptr;
    Scal<W> sm;
    scal_to_mont<W>(r, s_pre, 1, sm);
    for (size_t done = 0; done < batch; done += chunk) {
        const size_t now = std::min(chunk, batch - done);
        const W* src = reinterpret_cast<const W*>(in) + done * 3 * ew;
        if (pow_in) {
            if ((rc = crt_into<W>(r, win, {src}, 3 * now, false)) != ALCH_OK) return rc;
            src = reinterpret_cast<const W*>(win);
        }
        W* po = reinterpret_cast<W*>(out) + done * 2 * ew;
        ALCH_LAUNCH_VW(k_ct_split3, r, now * ew, r->stream, dev_ring<W>(r), src, po, c2pow, c2crt, now, sm, s_pre ? 1 : 0);
        HIP_TRY(hipGetLastError());
        if ((rc = do_crt<W>(r, c2pow, 0, now, true)) != ALCH_OK) return rc;
        if ((rc = ks_stage<W>(r, s, nullptr, nullptr, c2pow, po, now)) != ALCH_OK) return rc;
        if ((flags & ALCH_POW_OUT) && (rc = do_crt<W>(r, out, 2 * done, 2 * now, true)) != ALCH_OK) return rc;
    }
    return ALCH_OK;
}

extern "C" int alch_ct_key_switch_quad(const alch_hint* hint, const alch_buf* in, alch_buf* out, size_t batch, const uint64_t* s_pre,
                                       unsigned flags) try {
    if (!hint || !in || !out) return fail(ALCH_E_INVALID, "alch_ct_key_switch_quad: null argument");
    alch_ring* r = hint->ring;
    if (in->ring != r || out->ring != r) return fail(ALCH_E_INVALID, "alch_ct_key_switch_quad: the buffers must belong to the hint's ring");
    if (batch > in->n_elems / 3 || !pairs_ok(batch, out->n_elems))
        return fail(ALCH_E_INVALID, "alch_ct_key_switch_quad: in must hold 3*batch ring elements, out 2*batch");
    if (flags & ~(unsigned)(ALCH_POW_IN | ALCH_POW_OUT)) return fail(ALCH_E_INVALID, "alch_ct_key_switch_quad: unknown flag");
    if (out == in || bytes_overlap(out->dptr, 2 * batch * elem_bytes(r), in->dptr, 3 * batch * elem_bytes(r)))
        return fail(ALCH_E_INVALID, "alch_ct_key_switch_quad: out must not alias the input");
    if (!r->has_crt) return fail(ALCH_E_NO_CRT, "alch_ct_key_switch_quad: this ring has no CRT basis");
    if (batch == 0) return ALCH_OK;
    BIND(r);
    return ALCH_BY_WORD(r, do_key_switch_quad, r, hint, in->dptr, out->dptr, batch, s_pre, flags);
} catch (...) { return abi_catch(); }

// ---- the complete mul_: (*) . modSwitch up . keySwitchQuadCirc . modSwitch down -------------------------------
// Constants of the closing modSwitch that drops the first ddn limbs of `r` (outermost first): q_u^-1 mod q_t for the
// limb-at-a-time form, prod_{w >= u} q_w^-1 mod q_t for the forms that keep the surviving limbs in the CRT basis.
template <typename W>
static void fill_drop_tab(const alch_ring* r, int ddn, DropTab<W>& d) {
    d.ddn = ddn;
    d.balanced = 1;
    const int bits = 8 * (int)sizeof(W);
    for (int u = 0; u < MAXDROP; ++u)
        for (int t = 0; t < MAXL; ++t) { d.qinv_m[u][t] = 0; d.comb_m[u][t] = 0; }
    for (int u = 0; u < ddn; ++u)
        for (int t = u + 1; t < r->L; ++t) {
            const u64 qt = r->q[t], qu = r->q[u];
            if ((qu - 1) / 2 >= qt) d.balanced = 0;
            const u64 inv = h_powmod(qu % qt, qt - 2, qt);
            d.qinv_m[u][t] = (W)h_mulmod(inv, h_powmod(2, (u64)bits, qt), qt);
        }
    for (int u = 0; u < ddn; ++u)
        for (int t = ddn; t < r->L; ++t) {
            const u64 qt = r->q[t];
            u64 v = 1;
            for (int w = u; w < ddn; ++w) v = h_mulmod(v, h_powmod(r->q[w] % qt, qt - 2, qt), qt);
            d.comb_m[u][t] = (W)h_mulmod(v, h_powmod(2, (u64)bits, qt), qt);
        }
}

template <typename W>
static int do_mul_full(alch_ring* rh, alch_ring* rin, alch_ring* rout, const alch_hint* hint, const void* a, const void* b,
                       void* out, size_t batch, const uint64_t* s_pre, bool pow_out) {
    typedef typename Signed<W>::type SW;
    const int dup = rh->L - rin->L, ddn = rh->L - rout->L;
    const size_t n = rh->n;
    // per pipeline: digits [chunk][L_in][n] signed | key-switched chunk [chunk][2][Lh][n] | stash [slots][ddn][n] signed
    const size_t chunk = fused_chunk(rh->chunk, 2 * elem_bytes(rh), batch);                       // 32-bit byte offsets per array
    const unsigned slots = rh->rs_slots;       // resident workgroups of k_rescale_out (each owns a stash slot)
    const size_t dig_bytes = chunk * (size_t)rin->L * n * sizeof(SW);
    const size_t ks_bytes = chunk * 2 * (size_t)rh->L * n * sizeof(W);
    // stash: one slot per resident workgroup (k_rescale_out / _lin) or the lifted residues of the whole chunk (kernel_rescale_half.hpp)
    const size_t stash_bytes = std::max<size_t>(slots, 2 * chunk) * (size_t)ddn * n * sizeof(SW);
    const size_t pipe_bytes = dig_bytes + ks_bytes + stash_bytes;
    int rc = rh->ws_full.reserve(2 * pipe_bytes);
    if (rc != ALCH_OK) return rc;

    uint64_t s_eff[MAXL];                                  // s_pre times the moduli the first modSwitch adds
    for (int j = 0; j < rin->L; ++j) s_eff[j] = up_scalar(rh, dup, j + dup, s_pre ? s_pre[j] : 1);
    NttCall<W> c{};
    c.hint = reinterpret_cast<const W*>(hint->dptr);
    c.balanced = rh->balanced;
    c.opts = rh->opts;
    c.q30 = rh->q30 && rh->opts.q30;
    scal_to_mont<W>(rin, s_eff, 2, c.spre_r2);
    fill_drop_tab<W>(rh, ddn, c.drop);
    c.stash_slots = slots;
    c.pow_out = pow_out;

    const bool two = batch > chunk && !rh->one_stream;
    if (two) {
        HIP_TRY(hipEventRecord(rh->ev_fork, rh->stream));
        HIP_TRY(hipStreamWaitEvent(rh->aux, rh->ev_fork, 0));
    }
    const size_t in_words = 2 * (size_t)rin->L * n, out_words = 2 * (size_t)rout->L * n;
    size_t idx = 0;
    for (size_t done = 0; done < batch; done += chunk, ++idx) {
        const size_t now = std::min(chunk, batch - done);
        const bool odd = two && (idx & 1);
        char* base = reinterpret_cast<char*>(rh->ws_full.p) + (odd ? pipe_bytes : 0);
        c.stream = odd ? rh->aux : rh->stream;
        c.nct = now;
        // (*) 's quadratic coefficient, scaled, crtInv, TrivGad digits -- on the operands' ring
        c.op = OP_TENSOR_INTT;
        c.ring = &dev_ring<W>(rin);
        c.a = reinterpret_cast<const W*>(a) + done * in_words;
        c.b = reinterpret_cast<const W*>(b) + done * in_words;
        c.digits = base;
        if ((rc = launch(rh, c, "tensor_intt")) != ALCH_OK) return rc;
        // key switch on the hint's ring
        c.op = OP_KS_ACCUM;
        c.ring = &dev_ring<W>(rh);
        c.dup = dup;
        c.out = reinterpret_cast<W*>(base + dig_bytes);
        if ((rc = launch(rh, c, "ks_accum")) != ALCH_OK) return rc;
        // modSwitch down
        c.op = OP_RESCALE_OUT;
        c.a = reinterpret_cast<const W*>(base + dig_bytes);
        c.out = reinterpret_cast<W*>(out) + done * out_words;
        c.stash = base + dig_bytes + ks_bytes;
        if ((rc = launch(rh, c, "rescale_out")) != ALCH_OK) return rc;
    }
    if (two) {
        HIP_TRY(hipEventRecord(rh->ev_join, rh->aux));
        HIP_TRY(hipStreamWaitEvent(rh->stream, rh->ev_join, 0));
    }
    return ALCH_OK;
}

// ---- modSwitch down, the two composed forms: both queue on r's stream and write elements of ring_out, a suffix of r ----------
// CRT-resident form (general index, option rs_lin): the kept limbs stay in the CRT basis (k_gen_rescale_drop / k_gen_rescale_keep):
// ddn inverse + (L - ddn) forward transforms per component instead of L + (L - ddn).  res: ddn * n words of scratch per element.
template <typename W>
static int rescale_down_crt(alch_ring* r, int ddn, const void* in, void* res, void* out, size_t elems, bool dec_c0, bool pow_out,
                            size_t per = 2) {
    DropTab<W> dt;
    fill_drop_tab<W>(r, ddn, dt);
    const hipError_t e = gen_rescale_lin_dispatch(dev_ring<W>(r), gen_dev<W>(r), reinterpret_cast<const W*>(in), reinterpret_cast<W*>(res),
                                                  reinterpret_cast<W*>(out), dt, dec_c0 ? (int)per : 0, elems, r->stream, pow_out);   // c0 = every per-th element
    return e == hipSuccess ? ALCH_OK : fail(ALCH_E_HIP, std::string("rescale launch: ") + hipGetErrorString(e));
}

// Limb-at-a-time form.  cur: per * now elements of r on the Pow basis; c0 of every ciphertext (every per-th element) goes onto the Dec
// basis first for a general index (dec_c0, per = 2 or 3: rescaleDec).  The limbs are dropped outermost first through ping / pong (per * now elements each), the last step
// writes elements per * first .. of `out`; then back to the CRT basis on ring_out (same device tables as r's: queued on r's stream).
template <typename W>
static int rescale_down_limbs(alch_ring* r, alch_ring* rout, char* cur, char* ping, char* pong, void* out, size_t first, size_t now,
                              size_t per, bool dec_c0, bool pow_out) {
    const int ddn = r->L - rout->L;
    int rc;
    if (dec_c0 && (rc = do_columns<W>(r, GEN_LINV, cur, 0, now, per)) != ALCH_OK) return rc;
    for (int u = 0; u < ddn; ++u) {
        char* nxt = (u + 1 == ddn) ? reinterpret_cast<char*>(out) + first * per * elem_bytes(rout) : ((u & 1) ? pong : ping);
        const DevRing<W> rs = suffix_view<W>(r, u);
        const size_t total = per * now * (size_t)(rs.L - 1) * r->n;
        hipLaunchKernelGGL((k_rescale_drop0<W>), dim3(ew_grid(total)), dim3(256), 0, r->stream, rs, (const W*)cur, (W*)nxt, per * now,
                           drop0_inv_mont<W>(r, u));
        HIP_TRY(hipGetLastError());
        cur = nxt;
    }
    if (dec_c0 && (rc = do_columns<W>(rout, GEN_L, out, per * first, now, per, r)) != ALCH_OK) return rc;
    if (!pow_out && (rc = do_crt<W>(rout, out, per * first, per * now, false, nullptr, r)) != ALCH_OK) return rc;
    return ALCH_OK;
}

// The same mul_ for rings whose polynomial does not fit one LDS-resident transform (split crt, n = 2^16 / 2^15) and for general-index
// rings: the composed key switch on ring_h, then one of the composed modSwitch forms, one ciphertext chunk at a time.
template <typename W>
static int do_mul_full_unfused(alch_ring* rh, alch_ring* rin, alch_ring* rout, const alch_hint* hint, const void* a,
                               const void* b, void* out, size_t batch, const uint64_t* s_pre, bool pow_out) {
    const int L = rh->L, dup = L - rin->L, ddn = L - rout->L;
    const size_t eb = elem_bytes(rh);
    // scratch per ciphertext: key-switched pair (2) + the key-switch stage's (c2 in both bases + L digits, fewer for its one-kernel
    // forms) + rescale ping-pong (2 + 2), in ring_h elements
    KsStage<W> s = ks_stage_plan<W>(rh, hint, dup, false);
    const size_t per_ct = (2 + s.elems + 4) * eb;
    const size_t chunk = scratch_chunk(rh->scratch_mib << 20, batch, per_ct);
    int rc = rh->ws_full.reserve(chunk * per_ct);
    if (rc != ALCH_OK) return rc;
    Carve cv(rh->ws_full.p, chunk);
    char* ks = cv.take(2 * eb);
    ks_stage_carve(s, cv, eb);
    char *ping = cv.take(2 * eb), *pong = cv.take(2 * eb);
    if (!cv.matches(per_ct)) return fail(ALCH_E_INTERNAL, "do_mul_full_unfused: the scratch carve differs from the bytes reserved per ciphertext");
    uint64_t s_eff[MAXL];                                  // s_pre times the moduli the first modSwitch adds
    for (int j = 0; j < rin->L; ++j) s_eff[j] = up_scalar(rh, dup, j + dup, s_pre ? s_pre[j] : 1);
    scal_to_mont<W>(rin, s_eff, 2, s.sr2);
    const bool dec_c0 = rh->gen && rh->gh.rad > 1;     // general index: modSwitch rescales c0 on the Dec basis (rescaleDec), c1 on Pow
    const size_t in_words = 2 * elem_words(rin), out_bytes = 2 * elem_bytes(rout);
    for (size_t done = 0; done < batch; done += chunk) {
        const size_t now = std::min(chunk, batch - done);
        // (*), modSwitch up and keySwitchQuadCirc on ring_h
        if ((rc = ks_stage<W>(rh, s, reinterpret_cast<const W*>(a) + done * in_words, reinterpret_cast<const W*>(b) + done * in_words, nullptr,
                              reinterpret_cast<W*>(ks), now)) != ALCH_OK) return rc;
        // modSwitch down
        if (rh->gen && rh->opts.rs_lin && !pow_out)
            rc = rescale_down_crt<W>(rh, ddn, ks, ping, reinterpret_cast<char*>(out) + done * out_bytes, 2 * now, dec_c0, false);
        else if ((rc = do_crt<W>(rh, ks, 0, 2 * now, true)) == ALCH_OK)          // to the Pow basis first
            rc = rescale_down_limbs<W>(rh, rout, ks, ping, pong, out, done, now, 2, dec_c0, pow_out);
        if (rc != ALCH_OK) return rc;
    }
    return ALCH_OK;
}

static bool is_suffix_ring(const alch_ring* small, const alch_ring* big) {
    if (small->m != big->m || small->word != big->word || small->L >= big->L) return false;
    for (int j = 0; j < small->L; ++j)
        if (small->q[j] != big->q[big->L - small->L + j]) return false;
    return true;
}

// PT2CT's mul_ with a BaseBGad 2 hint whose ring has at least as many limbs as the operands': composed from the entry points'
// own implementations.  modSwitch up is linear and the tensor product bilinear, so  modSwitch (a * b) = (up a) * (up b) / q_a  on the
// old limbs and 0 on the added ones: both operands are switched up (alch_ct_mod_switch's kernel), the factor q_a^-1 rides on the
// tensor product's scalar, then the BaseBGad key switch of alch_ct_mul_relin and the closing alch_ct_mod_switch.
// A hint on FEWER limbs than the operands (KSPNoise (BaseBGad 2) = p + KSAccumPNoise can sit one limb below the product's
// p + MulPNoise): mul_full_base2_down below.
template <typename W> static int do_mod_switch(alch_ring* rin, alch_ring* rout, const void* in, void* out, size_t batch, unsigned flags, int per = 2);

// mul_ under a BaseBGad 2 hint that lives on FEWER limbs than the operands (PT2CT.hs:140,164: the product sits at p + MulPNoise units
// rounded up to whole limbs, the hint at p + KSAccumPNoise): the leading modSwitch goes DOWN on the quadratic ciphertext -- c0 on the
// decoding basis, c1 and c2 on the powerful basis -- before the key switch.
template <typename W>
static int mul_full_base2_down(const alch_hint* hint, alch_ring* rin, alch_ring* rh, const void* a, const void* b, void* ks, size_t batch,
                               const uint64_t* s_pre, alch_buf* t, alch_buf* c2, alch_buf* c2h) {
    Scal<W> sr2;
    scal_to_mont<W>(rin, s_pre, 2, sr2);
    const size_t words = batch * elem_words(rin);
    // the tensor product and both rescales run on the operands' stream, the key switch on the hint's
    ALCH_LAUNCH_VW(k_tensor_ew, rin, words, rin->stream, dev_ring<W>(rin), (const W*)a, (const W*)b, (W*)t->dptr, (W*)c2->dptr, batch, sr2, 0,
                   (W*)nullptr, g_table<W>(rin));
    HIP_TRY(hipGetLastError());
    int rc;
    if ((rc = do_mod_switch<W>(rin, rh, t->dptr, ks, batch, 0)) != ALCH_OK) return rc;
    if ((rc = do_mod_switch<W>(rin, rh, c2->dptr, c2h->dptr, batch, ALCH_POW_OUT, 1)) != ALCH_OK) return rc;
    HIP_TRY(hipStreamSynchronize(rin->stream));
    return do_mul_relin_unfused<W>(rh, hint, nullptr, nullptr, ks, batch, nullptr, c2h->dptr);
}
static int mul_full_base2(const alch_hint* hint, const alch_buf* a, const alch_buf* b, alch_buf* out, size_t batch, const uint64_t* s_pre,
                          unsigned flags) {
    alch_ring* rh = hint->ring;
    alch_ring* rin = a->ring;
    alch_ring* rout = out->ring;
    const bool in_down = rin->L > rh->L;                       // the leading modSwitch goes down, on the quadratic ciphertext
    auto same_ring = [](const alch_ring* x, const alch_ring* y) {           // another handle of the same (index, moduli)
        if (x->m != y->m || x->word != y->word || x->L != y->L) return false;
        for (int j = 0; j < x->L; ++j) if (x->q[j] != y->q[j]) return false;
        return true;
    };
    if (in_down ? !is_suffix_ring(rh, rin) : (!same_ring(rin, rh) && !is_suffix_ring(rin, rh)))
        return fail(ALCH_E_INVALID, "operand moduli must be the last limbs of the hint's ring, or the hint's the last limbs of the operands' (same word size)");
    if (in_down && !rin->has_crt) return fail(ALCH_E_NO_CRT, "the operands' ring has no CRT basis");
    if (!same_ring(rout, rh) && !is_suffix_ring(rout, rh)) return fail(ALCH_E_INVALID, "output moduli must be the last limbs of the hint's ring (same word size)");
    if (flags & ~(unsigned)ALCH_POW_OUT) return fail(ALCH_E_UNSUPPORTED, "only ALCH_POW_OUT is accepted");
    if (!rh->has_crt) return fail(ALCH_E_NO_CRT, "the hint's ring has no CRT basis");
    if (batch == 0) return ALCH_OK;
    if (!pairs_ok(batch, a->n_elems) || !pairs_ok(batch, b->n_elems) || !pairs_ok(batch, out->n_elems)) return fail(ALCH_E_INVALID, "buffers must hold 2*batch ring elements");
    if (bytes_overlap(out->dptr, 2 * batch * elem_bytes(rout), a->dptr, 2 * batch * elem_bytes(rin)) ||      // one ring may serve both sides
        bytes_overlap(out->dptr, 2 * batch * elem_bytes(rout), b->dptr, 2 * batch * elem_bytes(rin)))
        return fail(ALCH_E_INVALID, "alch_ct_mul_full: out must not alias an input");
    BIND(rh);
    const int dup = in_down ? 0 : rh->L - rin->L;
    alch_buf *ua = nullptr, *ub = nullptr, *ks = nullptr, *c2h = nullptr;
    int rc = ALCH_OK;
    auto done = [&](int code) {
        if (ua) alch_buf_free(ua); if (ub) alch_buf_free(ub); if (c2h) alch_buf_free(c2h); if (ks && ks != out) alch_buf_free(ks);
        return code;
    };
    // everything below is queued on ring_h's stream, behind the work of the other two rings
    HIP_TRY(hipStreamSynchronize(rin->stream));
    HIP_TRY(hipStreamSynchronize(rout->stream));
    const alch_buf *pa = a, *pb = b;
    uint64_t s_eff[MAXL];                                      // s_pre / q_a: each switched-up operand carries the added moduli, the product needs them once
    for (int j = 0; j < rh->L; ++j) s_eff[j] = j < dup ? 1 : up_scalar(rh, dup, j, s_pre ? s_pre[j - dup] : 1, true);
    if (dup > 0) {
        if ((rc = alch_buf_alloc(rh, 2 * batch, &ua)) != ALCH_OK || (rc = alch_buf_alloc(rh, 2 * batch, &ub)) != ALCH_OK) return done(rc);
        // alch_ct_mod_switch up works on rout's stream = rh's here
        rc = ALCH_BY_WORD(rh, do_mod_switch, rin, rh, a->dptr, ua->dptr, batch, 0);
        if (rc == ALCH_OK) rc = ALCH_BY_WORD(rh, do_mod_switch, rin, rh, b->dptr, ub->dptr, batch, 0);
        if (rc != ALCH_OK) return done(rc);
        pa = ua; pb = ub;
    }
    const bool down = rout->L < rh->L;
    if (down || (flags & ALCH_POW_OUT)) { if ((rc = alch_buf_alloc(rh, 2 * batch, &ks)) != ALCH_OK) return done(rc); }
    else ks = out;
    if (in_down) {
        // ua: the (c0, c1) pairs, ub: c2, both on the operands' ring; c2h: c2 on the hint's ring, powerful basis
        if ((rc = alch_buf_alloc(rin, 2 * batch, &ua)) != ALCH_OK || (rc = alch_buf_alloc(rin, batch, &ub)) != ALCH_OK ||
            (rc = alch_buf_alloc(rh, batch, &c2h)) != ALCH_OK) return done(rc);
        HIP_TRY(hipStreamSynchronize(rh->stream));
        rc = ALCH_BY_WORD(rh, mul_full_base2_down, hint, rin, rh, a->dptr, b->dptr, ks->dptr, batch, s_pre, ua, ub, c2h);
    } else
        rc = ALCH_BY_WORD(rh, do_mul_relin_unfused, rh, hint, pa->dptr, pb->dptr, ks->dptr, batch, s_eff);
    if (rc != ALCH_OK) return done(rc);
    if (down) {
        rc = ALCH_BY_WORD(rh, do_mod_switch, rh, rout, ks->dptr, out->dptr, batch, flags & ALCH_POW_OUT);
    } else if (flags & ALCH_POW_OUT) {
        HIP_TRY(hipMemcpyAsync(out->dptr, ks->dptr, 2 * batch * elem_bytes(rh), hipMemcpyDeviceToDevice, rh->stream));
        rc = ALCH_BY_WORD(rh, do_crt, rh, out->dptr, 0, 2 * batch, true);
    }
    if (rc != ALCH_OK) return done(rc);
    HIP_TRY(hipStreamSynchronize(rh->stream));                 // the scratch buffers are freed on return
    return done(ALCH_OK);
}

extern "C" int alch_ct_mul_full(const alch_hint* hint, const alch_buf* a, const alch_buf* b, alch_buf* out, size_t batch,
                                const uint64_t* s_pre, unsigned flags) try {
    if (!hint || !a || !b || !out) return fail(ALCH_E_INVALID, "null argument");
    alch_ring* rh = hint->ring;
    alch_ring* rin = a->ring;
    alch_ring* rout = out->ring;
    if (b->ring != rin) return fail(ALCH_E_INVALID, "operands belong to different rings");
    if (gadget_width(hint->gadget) > 0) return mul_full_base2(hint, a, b, out, batch, s_pre, flags);
    if (!is_suffix_ring(rin, rh)) return fail(ALCH_E_INVALID, "operand moduli must be the last limbs of the hint's ring (same word size)");
    if (!is_suffix_ring(rout, rh)) return fail(ALCH_E_INVALID, "output moduli must be the last limbs of the hint's ring (same word size)");
    if (rh->L - rout->L > MAXDROP) return fail(ALCH_E_UNSUPPORTED, "at most 3 limbs dropped per call");
    if (flags & ~(unsigned)ALCH_POW_OUT) return fail(ALCH_E_UNSUPPORTED, "only ALCH_POW_OUT is accepted");
    if (batch == 0) return ALCH_OK;
    BIND(rh);
    if (!pairs_ok(batch, a->n_elems) || !pairs_ok(batch, b->n_elems) || !pairs_ok(batch, out->n_elems))
        return fail(ALCH_E_INVALID, "buffers must hold 2*batch ring elements");
    // operands and output may live on ONE suffix ring of the hint's (mul_ at q: up to q', key switch, down to q), so out can be a
    // view into an operand: refused by bytes, as in alch_ct_mul_relin
    if (bytes_overlap(out->dptr, 2 * batch * elem_bytes(rout), a->dptr, 2 * batch * elem_bytes(rin)) ||
        bytes_overlap(out->dptr, 2 * batch * elem_bytes(rout), b->dptr, 2 * batch * elem_bytes(rin)))
        return fail(ALCH_E_INVALID, "alch_ct_mul_full: out must not alias an input");
    // everything runs on the hint ring's stream, behind the work of the other two rings (one wait serves both where they share a stream)
    const bool two_others = rout->stream != rin->stream;
    int rc;
    if ((rc = ext_order(rh, rin, true)) != ALCH_OK) return rc;
    if (two_others && (rc = ext_order(rh, rout, true)) != ALCH_OK) return rc;
    const bool pow_out = (flags & ALCH_POW_OUT) != 0;
    if (!rh->has_crt) return fail(ALCH_E_NO_CRT, "the hint's ring has no CRT basis");
    if (split_ring(rh) || rh->gen)
        rc = ALCH_BY_WORD(rh, do_mul_full_unfused, rh, rin, rout, hint, a->dptr, b->dptr, out->dptr, batch, s_pre, pow_out);
    else
        rc = ALCH_BY_WORD(rh, do_mul_full, rh, rin, rout, hint, a->dptr, b->dptr, out->dptr, batch, s_pre, pow_out);
    if (rc != ALCH_OK) return rc;
    if ((rc = ext_order(rh, rin, false)) != ALCH_OK) return rc;
    return two_others ? ext_order(rh, rout, false) : ALCH_OK;
} catch (...) { return abi_catch(); }

// ------------------------------------------------------------------------------------------------------
// ring tunnelling: tunnel_ hint between two modSwitch_ (PT2CT.hs:224-229, Eval.hs:134)
// ------------------------------------------------------------------------------------------------------
extern "C" int alch_tunnel_info(const alch_ring* rr, const alch_ring* rs, uint32_t* e_prime, uint32_t* d_rel) try {
    if (!rr || !rs) return fail(ALCH_E_INVALID, "null ring");
    if (!rr->gen && !rs->gen) {                  // two two-power indices >= 32: every such pair is a tunnel, E' is the smaller ring
        if (e_prime) *e_prime = std::min(rr->m, rs->m);
        if (d_rel) *d_rel = rr->m > rs->m ? rr->m / rs->m : 1u;
        return ALCH_OK;
    }
    u32 a = rr->m, b = rs->m;
    while (b) { const u32 t = a % b; a = b; b = t; }
    GenHost ge, gr, gs;
    if (!gen_plan(a, ge) || !gen_plan(rr->m, gr) || !gen_plan(rs->m, gs)) return fail(ALCH_E_UNSUPPORTED, "index not served");
    u32 d = 0, mask = 0;
    std::vector<int32_t> tab;
    if (!gen_tunnel_table(ge, gr, gs, d, tab, mask)) return fail(ALCH_E_INVALID, "indices do not form a tunnel");
    if (e_prime) *e_prime = a;
    if (d_rel) *d_rel = d;
    return ALCH_OK;
} catch (...) { return abi_catch(); }

template <typename W>
static int tunnel_to_mont(alch_ring* rs, void* dst, const void* src, size_t elems) {
    Scal<W> sm;
    scal_to_mont<W>(rs, nullptr, 2, sm);
    const size_t words = elems * elem_words(rs);
    ALCH_LAUNCH_VW(k_scale, rs, words, rs->stream, dev_ring<W>(rs), (W*)dst, (const W*)src, words, sm);
    HIP_TRY(hipGetLastError());
    return ALCH_OK;
}

extern "C" int alch_tunnel_create(alch_ring* rr, alch_ring* rs, int gadget, const alch_buf* lin_crt, const alch_buf* ks_crt, alch_tunnel** out) try {
    if (!rr || !rs || !lin_crt || !ks_crt || !out) return fail(ALCH_E_INVALID, "null argument");
    *out = nullptr;
    if (gadget_width(gadget) < 0) return fail(ALCH_E_INVALID, "alch_tunnel_create: unknown gadget");
    if (!rr->has_crt || !rs->has_crt) return fail(ALCH_E_UNSUPPORTED, "tunnelling runs on rings with a CRT basis");
    if (rr->gen != rs->gen)
        return fail(ALCH_E_UNSUPPORTED, "tunnelling between a two-power ring with m >= 32 and a general-index ring (composite m, or two-power m < 32) is not served");
    if (rr->L != rs->L || rr->word != rs->word) return fail(ALCH_E_INVALID, "both rings must have the same moduli");
    for (int j = 0; j < rr->L; ++j) if (rr->q[j] != rs->q[j]) return fail(ALCH_E_INVALID, "both rings must have the same moduli");
    if (lin_crt->ring != rs || ks_crt->ring != rs) return fail(ALCH_E_INVALID, "the linear function and the hints live in the target ring");
    u32 ep = 0, d_rel = 0;
    int rc = alch_tunnel_info(rr, rs, &ep, &d_rel);
    if (rc != ALCH_OK) return rc;
    if (!rr->gen) {                              // two-power rings of the radix-16 engine: no index tables (do_tunnel_pow2)
        const int digits = gadget_digits(rs, gadget);
        const size_t nlin = d_rel, nks = (size_t)d_rel * (size_t)digits * 2;
        if (lin_crt->n_elems < nlin || ks_crt->n_elems < nks)
            return fail(ALCH_E_INVALID, "need d_rel linear-function values and 2 * d_rel * (gadget digits) hint elements");
        BIND(rs);
        alch_tunnel* t = new alch_tunnel{rr, rs, d_rel, 0, nullptr, nullptr, nullptr, gadget, digits};
        t->pow2 = true;
        for (u32 r = rr->n; r < rs->n; r <<= 1) ++t->sh;
        if (hipMalloc(&t->lin, nlin * elem_bytes(rs)) != hipSuccess || hipMalloc(&t->ks, nks * elem_bytes(rs)) != hipSuccess) {
            alch_tunnel_free(t);
            return fail(ALCH_E_NOMEM, "hipMalloc(tunnel) failed");
        }
        rc = ALCH_BY_WORD(rs, tunnel_to_mont, rs, t->lin, lin_crt->dptr, nlin);
        if (rc == ALCH_OK) rc = ALCH_BY_WORD(rs, tunnel_to_mont, rs, t->ks, ks_crt->dptr, nks);
        if (rc != ALCH_OK) { alch_tunnel_free(t); return rc; }
        if (hipStreamSynchronize(rs->stream) != hipSuccess) { alch_tunnel_free(t); return fail(ALCH_E_HIP, "tunnel setup failed"); }
        *out = t;
        return ALCH_OK;
    }
    GenHost ge;
    gen_plan(ep, ge);
    std::vector<int32_t> tab, tab_e;
    std::vector<u32> slot_e;
    u32 mask = 0;
    if (!gen_tunnel_table(ge, rr->gh, rs->gh, d_rel, tab, mask, &tab_e, &slot_e)) return fail(ALCH_E_INVALID, "indices do not form a tunnel");
    const int digits = gadget_digits(rs, gadget);
    const size_t nlin = d_rel, nks = (size_t)d_rel * (size_t)digits * 2;
    if (lin_crt->n_elems < nlin || ks_crt->n_elems < nks)
        return fail(ALCH_E_INVALID, "need d_rel linear-function values and 2 * d_rel * (gadget digits) hint elements");
    BIND(rs);
    alch_tunnel* t = new alch_tunnel{rr, rs, d_rel, mask, nullptr, nullptr, nullptr, gadget, digits};
    if (hipMalloc((void**)&t->table, tab.size() * sizeof(int32_t)) != hipSuccess ||
        hipMalloc(&t->lin, nlin * elem_bytes(rs)) != hipSuccess || hipMalloc(&t->ks, nks * elem_bytes(rs)) != hipSuccess) {
        alch_tunnel_free(t);
        return fail(ALCH_E_NOMEM, "hipMalloc(tunnel) failed");
    }
    if (hipMemcpy(t->table, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) { alch_tunnel_free(t); return fail(ALCH_E_HIP, "tunnel table upload failed"); }
    if (ep != rs->m && rs->opts.tunnel_ep) {           // E' smaller than S': run the transforms there when E' has a general-index ring
        alch_ring* re = nullptr;
        if (alch_ring_create(ep, rs->L, rs->q, &re) == ALCH_OK && re->gen && re->word == rs->word && re->n % 4 == 0 && rs->n % 4 == 0) {
            t->re = re;
            re->g32.nt = rs->g32.nt; re->g64.nt = rs->g64.nt;      // launch-structure options of the target ring apply to its E' ring
            t->pieces_ok = true;
            for (size_t k = 0; k + 3 < slot_e.size(); k += 4)
                if (slot_e[k] % 4 || slot_e[k + 1] != slot_e[k] + 1 || slot_e[k + 2] != slot_e[k] + 2 || slot_e[k + 3] != slot_e[k] + 3) { t->pieces_ok = false; break; }
            if (hipMalloc((void**)&t->table_e, tab_e.size() * sizeof(int32_t)) != hipSuccess ||
                hipMalloc((void**)&t->slot_e, slot_e.size() * sizeof(u32)) != hipSuccess ||
                hipMemcpy(t->table_e, tab_e.data(), tab_e.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(t->slot_e, slot_e.data(), slot_e.size() * sizeof(u32), hipMemcpyHostToDevice) != hipSuccess) {
                alch_tunnel_free(t);
                return fail(ALCH_E_NOMEM, "hipMalloc(tunnel, E' tables) failed");
            }
        } else if (re) {
            alch_ring_destroy(re);
        }
        BIND(rs);
    }
    rc = ALCH_BY_WORD(rs, tunnel_to_mont, rs, t->lin, lin_crt->dptr, nlin);
    if (rc == ALCH_OK) rc = ALCH_BY_WORD(rs, tunnel_to_mont, rs, t->ks, ks_crt->dptr, nks);
    if (rc != ALCH_OK) { alch_tunnel_free(t); return rc; }
    if (hipStreamSynchronize(rs->stream) != hipSuccess) { alch_tunnel_free(t); return fail(ALCH_E_HIP, "tunnel setup failed"); }
    *out = t;
    return ALCH_OK;
} catch (...) { return abi_catch(); }

extern "C" int alch_tunnel_free(alch_tunnel* t) try {
    if (!t) return ALCH_OK;
    (void)hipSetDevice(t->rs->device);
    (void)hipStreamSynchronize(t->rs->stream);
    if (t->table) (void)hipFree(t->table);
    if (t->lin) (void)hipFree(t->lin);
    if (t->ks) (void)hipFree(t->ks);
    if (t->table_e) (void)hipFree(t->table_e);
    if (t->slot_e) (void)hipFree(t->slot_e);
    if (t->re) alch_ring_destroy(t->re);
    delete t;
    return ALCH_OK;
} catch (...) { return abi_catch(); }

// The digit tail of a general-index key-switch stage (do_tunnel, do_hoisted): `coeffs` embedded coefficients in x1 ([coeff][Lx][n], the
// limbs xoff .. xoff + Lx - 1) at the transforms' ring rx, queued on rs's stream; dig receives the crt of their GD digits each,
// decomposed and reduced in the transforms' loader -- BaseBGad 2^bw (bw > 0; examples/Tunnel.hs:24) or TrivGad (GD = Lx).
template <typename W>
static int gen_digit_tail(alch_ring* rs, alch_ring* rx, const char* x1, char* dig, size_t coeffs, u32 GD, u32 Lx, u32 xoff, u32 bw,
                          const Scal<u32>& b2first, const Scal<u32>& b2kd) {
    GenCall<W> g{};
    g.ring = &dev_ring<W>(rx); g.gen = &gen_dev<W>(rx); g.stream = rs->stream;
    g.src = reinterpret_cast<const W*>(x1); g.data = reinterpret_cast<W*>(dig);
    if (bw > 0) {
        g.op = GEN_CRT_BASE2;
        g.npoly = coeffs * (size_t)GD * (size_t)rs->L; g.b2_first = b2first; g.b2_kd = b2kd; g.b2_D = GD; g.b2_w = bw;
        return launch(g, "tunnel base2 crt_digits");
    }
    g.op = GEN_CRT_DIGITS;
    g.npoly = coeffs * (size_t)Lx * (size_t)rs->L; g.balanced = rs->balanced; g.with_diag = true;
    g.src_limbs = (int)Lx; g.src_first = (int)xoff;
    return launch(g, "tunnel crt_digits");
}

// SymmSHE.tunnel on a batch of linear ciphertexts (k = 0):  out = (f'(c0), 0) + sum_i switch(hint_i, embed(c1_i)).
// rin: the ring the ciphertexts live in -- the tunnel's R' ring or its last limbs (PT2CT emits modSwitch_ .: tunnel_ hint .: modSwitch_,
// PT2CT.hs:224-229; the leading modSwitch up, x -> (0, q_a x), is then folded in: the added limbs are zero, so neither their
// crtInv, nor the crt of their embedded constant terms, nor their digits' transforms and hint products are computed).
template <typename W>
static int do_tunnel(const alch_tunnel* t, alch_ring* rin, const void* in, void* out, size_t batch, const uint64_t* s_pre, unsigned flags) {
    alch_ring* rr = t->rr;
    alch_ring* rs = t->rs;
    const int L = rs->L, dup = rr->L - rin->L;
    const u32 D = t->d_rel;
    const u32 bw = (u32)gadget_width(t->gadget);     // BaseBGad 2^bw; 0: TrivGad
    const bool base2 = bw > 0;
    // compact: embedded coefficients and digits hold the L - dup non-zero limbs only (TrivGad; BaseBGad 2 keeps the
    // full layout with explicit zero limbs)
    const bool compact = dup > 0 && !base2;
    const u32 Lx = compact ? (u32)(L - dup) : (u32)L, xoff = compact ? (u32)dup : 0u;
    const u32 GD = base2 ? (u32)t->digits : Lx;     // gadget digits per embedded coefficient
    Scal<u32> b2first, b2kd;
    if (base2) base2_layout(rs, b2first, b2kd, bw);
    // rx: the ring the E'-coefficients are transformed in -- E' itself when the tunnel has its ring (the CRT over S' of an embedded
    // element is its CRT over E' replicated: k_tunnel_lin / k_hint_mac read it through slot_e), else S' with the coefficients embedded
    alch_ring* rx = t->re ? t->re : rs;
    const u32* slot_e = t->re ? t->slot_e : nullptr;
    const size_t ebr = elem_bytes(rin), ebs = elem_bytes(rs), ebd = elem_bytes(rx), ebx = ebd / (size_t)L * Lx;
    // TrivGad, 32-bit words, E'-level transforms with piece-aligned slot table: digit transforms + hint products fused (k_gen_tunnel_ks)
    const bool fused = sizeof(W) == 4 && !base2 && t->re && t->pieces_ok && rs->opts.tunnel_fused && rs->n % 4 == 0 && rx->n % 4 == 0 &&
                       rs->n <= (u32)(GEN_TUN_T * 4 * 6) && 2 * (size_t)rx->n * sizeof(W) <= 65536;
    const int tun_ng = (rs->opts.tunnel_fused == 4 && 4 * (size_t)rx->n * sizeof(W) <= 65536) ? 4 : 2;     // two workgroups per CU: 64 KiB of LDS each
    // scratch per ciphertext: Pow copy of the input (2 R'-elements), x0, x1 (D coefficients each), digits (D * GD elements of rx)
    const size_t per_ct = 2 * ebr + 2 * (size_t)D * ebx + (fused ? 0 : (size_t)D * GD * ebd);
    const size_t chunk = scratch_chunk(rs->scratch_mib << 20, batch, per_ct);
    int rc = rs->ws_full.reserve(chunk * per_ct);
    if (rc != ALCH_OK) return rc;
    Carve cv(rs->ws_full.p, chunk);
    char *win = cv.take(2 * ebr), *x0 = cv.take(D * ebx), *x1 = cv.take(D * ebx), *dig = cv.take(fused ? 0 : (size_t)D * GD * ebd);
    if (!cv.matches(per_ct)) return fail(ALCH_E_INTERNAL, "do_tunnel: the scratch carve differs from the bytes reserved per ciphertext");
    uint64_t s_eff[MAXL] = {0};
    for (int j = dup; j < L; ++j) s_eff[j] = up_scalar(rs, dup, j, s_pre ? s_pre[j] : 1);      // modSwitch up: times the added moduli
    const bool scale = s_pre != nullptr || dup > 0;
    Scal<W> sm;
    scal_to_mont<W>(rs, s_eff, 1, sm);
    const bool dec_c0 = rr->gh.rad > 1 && t->linv_skip_mask != ((1u << rr->gh.nfact) - 1);
    for (size_t done = 0; done < batch; done += chunk) {
        const size_t now = std::min(chunk, batch - done);
        const char* src = reinterpret_cast<const char*>(in) + done * 2 * ebr;
        // Pow basis of R' (a copy: the caller's ciphertexts are left alone); c0 onto relative-Dec (x) Pow(E')
        // Pow-basis input is read in place (c1 always; c0 through an out-of-place lInv into the scratch when the tunnel needs one)
        const bool pin = (flags & ALCH_POW_IN) != 0;
        if (!pin && (rc = do_crt<W>(rin, win, 0, 2 * now, true, src, rs)) != ALCH_OK) return rc;
        if (dec_c0) {
            GenCall<W> g{};
            g.op = GEN_LINV; g.ring = &dev_ring<W>(rin); g.gen = &gen_dev<W>(rin); g.stream = rs->stream;
            g.data = reinterpret_cast<W*>(win); g.src = pin ? reinterpret_cast<const W*>(src) : nullptr;
            g.elem_stride = 2; g.first_poly = 0; g.npoly = now * (size_t)rin->L;
            g.skip_mask = t->linv_skip_mask; g.fail_flag = rin->d_flag;
            if ((rc = launch(g, "tunnel lInv")) != ALCH_OK) return rc;
        }
        const W* in0 = (pin && !dec_c0) ? reinterpret_cast<const W*>(src) : reinterpret_cast<const W*>(win);
        const W* in1 = pin ? reinterpret_cast<const W*>(src) : reinterpret_cast<const W*>(win);
        const size_t gw = now * 2 * (size_t)D * Lx * rx->n;
        ALCH_LAUNCH_VW(k_tunnel_gather, rx, gw, rs->stream, dev_ring<W>(rx), in0, in1, (W*)x0, (W*)x1,
                           t->re ? t->table_e : t->table, D, rr->n, now, sm, scale ? 1 : 0, Lx, xoff, (u32)dup);
        HIP_TRY(hipGetLastError());
        // constant term: evalLin
        if (compact) {
            DevRing<W> dv; GenDev<W> gv;
            gen_suffix_view<W>(rx, dup, dv, gv);
            GenCall<W> g{};
            g.op = GEN_CRT; g.ring = &dv; g.gen = &gv; g.stream = rs->stream;
            g.data = reinterpret_cast<W*>(x0); g.first_poly = 0; g.npoly = now * (size_t)D * Lx;
            if ((rc = launch(g, "tunnel crt")) != ALCH_OK) return rc;
        } else if ((rc = do_crt<W>(rx, x0, 0, now * D, false, nullptr, rs)) != ALCH_OK) return rc;
        W* po = reinterpret_cast<W*>(reinterpret_cast<char*>(out) + done * 2 * ebs);
        // k_tunnel_mac_e starts its accumulators from evalLin's constant term itself: no pass for it then
        const bool mac_e = sizeof(W) == 4 && !fused && (slot_e ? t->pieces_ok : true) && rs->n % 4 == 0 && rx->n % 4 == 0 && rs->opts.tunnel_mac;
        if (!mac_e) {
            ALCH_LAUNCH_VW(k_tunnel_lin, rs, now * elem_words(rs), rs->stream, dev_ring<W>(rs), po, (const W*)x0,
                           (const W*)t->lin, D, now, Lx, xoff, slot_e, rx->n);
            HIP_TRY(hipGetLastError());
        }
        // linear term: decompose + reduce + crt of every embedded coefficient, inner product with the hints
        if (fused) {                                  // one kernel, no digits in HBM (k_gen_tunnel_ks)
            if constexpr (sizeof(W) == 4) {
                GenTunArgs<u32> A{};
                A.x1 = reinterpret_cast<const u32*>(x1); A.hint = reinterpret_cast<const u32*>(t->ks); A.out = reinterpret_cast<u32*>(po);
                A.slot_e = slot_e; A.D = D; A.Lx = Lx; A.xoff = xoff; A.n_s = rs->n; A.balanced = rs->balanced ? 1 : 0;
                hipError_t e = gen_tunnel_ks_dispatch(rs->d32, rx->g32, A, now, tun_ng, rs->stream);
                if (e != hipSuccess) return fail(ALCH_E_HIP, std::string("fused tunnel key switch launch: ") + hipGetErrorString(e));
            }
            continue;
        }
        if ((rc = gen_digit_tail<W>(rs, rx, x1, dig, now * (size_t)D, GD, Lx, xoff, bw, b2first, b2kd)) != ALCH_OK) return rc;
        if (mac_e) {
            if constexpr (sizeof(W) == 4) {
                const size_t pieces = (now + 3) / 4 * (size_t)rs->L * (rs->n / 4);
                hipLaunchKernelGGL((k_tunnel_mac_e<4>), dim3(ew_grid(pieces)), dim3(256), 0, rs->stream, rs->d32, (u32*)po, (const u32*)dig, (const u32*)t->ks,
                                   now, D * GD, Lx, compact ? (u32)dup : 0u, slot_e, rx->n, (const u32*)x0, (const u32*)t->lin, D, Lx, xoff);
            }
        } else {
            launch_hint_mac<W>(rs, rs->stream, po, (const W*)dig, (const W*)t->ks, now, D * GD, (const W*)nullptr, Lx, compact ? (u32)dup : 0u,
                               slot_e, rx->n, t->pieces_ok);
        }
        HIP_TRY(hipGetLastError());
    }
    return ALCH_OK;
}

// crt / crtInv in place of `count` elements that hold only the last L - u limbs of two-power ring r ([elem][L - u][n])
template <typename W>
static int crt_suffix(alch_ring* r, int u, void* data, size_t count, bool inverse, const alch_ring* on) {
    if (u == 0) return do_crt<W>(r, data, 0, count, inverse, nullptr, on);
    const DevRing<W> dv = suffix_view<W>(r, u);
    NttCall<W> c{};
    c.op = inverse ? OP_CRTINV : OP_CRT;
    c.ring = &dv; c.stream = on->stream; c.data = reinterpret_cast<W*>(data);
    c.first_poly = 0; c.npoly = count * (size_t)dv.L;
    return launch(r, c, "crt");
}

template <typename W, bool TRIV>
static void launch_tun2_gather(alch_ring* rs, u32 d, const W* in, W* x0, W* dst1, u32 n_d, size_t nct, const Scal<W>& sm, bool scale, u32 dup) {
    constexpr int VL = Vec4<W>::LANES;
    const u32 g = d < (u32)VL ? d : (u32)VL;
    const size_t items = nct * (x0 ? 2 : 1) * (size_t)(TRIV ? rs->L - (int)dup : rs->L) * (d / g) * (n_d / VL);
    const dim3 grid(ew_grid(items)), block(256);
    const int bal = rs->balanced ? 1 : 0, sc = scale ? 1 : 0;
    if (g == 1) hipLaunchKernelGGL((k_tun2_gather<W, 1, TRIV>), grid, block, 0, rs->stream, dev_ring<W>(rs), in, x0, dst1, d, n_d, nct, sm, sc, dup, bal);
    else if (g == 2) hipLaunchKernelGGL((k_tun2_gather<W, 2, TRIV>), grid, block, 0, rs->stream, dev_ring<W>(rs), in, x0, dst1, d, n_d, nct, sm, sc, dup, bal);
    else hipLaunchKernelGGL((k_tun2_gather<W, VL, TRIV>), grid, block, 0, rs->stream, dev_ring<W>(rs), in, x0, dst1, d, n_d, nct, sm, sc, dup, bal);
}

// The digit tail of a two-power key-switch stage, `elems` coefficient elements at the transforms' ring rd, queued on ring `on`'s stream
// (do_tunnel_pow2, do_hoisted).  BaseBGad 2^bw (bw > 0): x1 holds the elements ([elem][L][n_d]) and dig receives the crt of their GD
// digits each -- decomposed and reduced in the transforms' loader (OP_CRT_BASE2) or, on split rings, by k_decompose_base2 + do_crt.
// TrivGad (bw = 0): dig holds the digits already (k_tun2_gather wrote them decomposed and reduced) and takes one batched crt.
template <typename W>
static int pow2_digit_tail(alch_ring* rd, alch_ring* on, const char* x1, char* dig, size_t elems, u32 GD, u32 bw, const Scal<u32>& b2first,
                           const Scal<u32>& b2kd) {
    int rc;
    if (bw > 0 && !split_ring(rd)) {
        NttCall<W> nc{};
        nc.op = OP_CRT_BASE2; nc.ring = &dev_ring<W>(rd); nc.stream = on->stream; nc.balanced = rd->balanced;
        nc.src = reinterpret_cast<const W*>(x1); nc.data = reinterpret_cast<W*>(dig);
        nc.npoly = elems * GD * (size_t)rd->L;
        nc.b2_first = b2first; nc.b2_kd = b2kd; nc.b2_D = GD; nc.b2_w = bw;
        return launch(rd, nc, "tunnel crt_base2");
    }
    if (bw > 0) {
        for (size_t y0 = 0; y0 < elems; y0 += 32768) {             // grid.y is 16-bit
            const unsigned ny = (unsigned)std::min<size_t>(32768, elems - y0);
            launch_decompose_baseb<W>(rd, on->stream, dev_ring<W>(rd), ny, reinterpret_cast<const W*>(x1) + y0 * elem_words(rd),
                                      reinterpret_cast<W*>(dig) + y0 * GD * elem_words(rd), b2first, b2kd, GD, bw);
            HIP_TRY(hipGetLastError());
        }
    }
    if ((rc = do_crt<W>(rd, dig, 0, elems * GD, false, nullptr, on)) != ALCH_OK) return rc;
    return ALCH_OK;
}

// SymmSHE.tunnel between two two-power rings of the radix-16 engine (m >= 32 on both sides); same contract as do_tunnel.  Two shapes:
//   up    R' = E' inside S' (d_rel = 1): coeffs is the identity and everything is transformed at dimension n_r -- crtInv of the input,
//         the digits' crt -- while the products with the linear function and the hints read slot k >> sh (k_tun2_mac).  CRT input: c0 is
//         read where it lies, no gather and no transform for it.
//   down  R' over S' = E' (d_rel = n_r / n_s): crtInv at R', the stride-d_rel gather, d_rel (1 + D) transforms at n_s, sh = 0.
// g = 1 and l = identity on a two-power index: no lInv / l step.  The digit tail follows ks_stage's ladder for two-power rings: BaseBGad 2
// in the transforms' loader (OP_CRT_BASE2) or, on split rings, k_decompose_base2 + do_crt; TrivGad digits leave the gather already
// decomposed and reduced (compact: only the L - dup limbs the input has) and take one batched crt.
template <typename W>
static int do_tunnel_pow2(const alch_tunnel* t, alch_ring* rin, const void* in, void* out, size_t batch, const uint64_t* s_pre, unsigned flags) {
    alch_ring* rr = t->rr;
    alch_ring* rs = t->rs;
    const int L = rs->L, dup = rr->L - rin->L, Lin = L - dup;
    const u32 d = t->d_rel;
    const u32 bw = (u32)gadget_width(t->gadget);      // BaseBGad 2^bw; 0: TrivGad
    const bool base2 = bw > 0, up = rs->n > rr->n, pin = (flags & ALCH_POW_IN) != 0;
    alch_ring* rd = up ? rr : rs;                      // the ring whose dimension the transforms run at
    const u32 n_d = rd->n;
    const bool c0_in_place = up && !pin;               // crt_S'(embed c0)[k] = crt_R'(c0)[k >> sh]: the input's CRT form serves as it is
    const u32 GD = base2 ? (u32)t->digits : (u32)Lin;  // digits per E'-coefficient
    Scal<u32> b2first, b2kd;
    if (base2) base2_layout(rs, b2first, b2kd, bw);
    const size_t wb = sizeof(W), ebr = elem_bytes(rin), pd = (size_t)n_d * wb;        // pd: one limb-polynomial at the transforms' dimension
    const size_t x0_b = c0_in_place ? 0 : (size_t)d * Lin * pd, x1_b = base2 ? (size_t)d * L * pd : 0, dig_b = (size_t)d * GD * L * pd;
    const size_t per_ct = 2 * ebr + x0_b + x1_b + dig_b;
    const size_t chunk = scratch_chunk(rs->scratch_mib << 20, batch, per_ct);
    int rc = rs->ws_full.reserve(chunk * per_ct);
    if (rc != ALCH_OK) return rc;
    Carve cv(rs->ws_full.p, chunk);
    char *win = cv.take(2 * ebr), *x0 = cv.take(x0_b), *x1 = cv.take(x1_b), *dig = cv.take(dig_b);
    if (!cv.matches(per_ct)) return fail(ALCH_E_INTERNAL, "do_tunnel_pow2: the scratch carve differs from the bytes reserved per ciphertext");
    uint64_t s_eff[MAXL] = {0};
    for (int j = dup; j < L; ++j) s_eff[j] = up_scalar(rs, dup, j, s_pre ? s_pre[j] : 1);      // modSwitch up: times the added moduli
    const bool scale = s_pre != nullptr || dup > 0;
    Scal<W> sm;
    scal_to_mont<W>(rs, s_eff, 1, sm);
    const size_t ebs = elem_bytes(rs);
    for (size_t done = 0; done < batch; done += chunk) {
        const size_t now = std::min(chunk, batch - done);
        const char* src = reinterpret_cast<const char*>(in) + done * 2 * ebr;
        // Pow basis of R' (a copy: the caller's ciphertexts are left alone); Pow-basis input is read in place
        if (!pin && (rc = crt_into<W>(rin, win, {src}, 2 * now, true, rs)) != ALCH_OK) return rc;
        const W* pow_in = reinterpret_cast<const W*>(pin ? src : win);
        W* px0 = c0_in_place ? nullptr : reinterpret_cast<W*>(x0);
        if (base2) launch_tun2_gather<W, false>(rs, d, pow_in, px0, reinterpret_cast<W*>(x1), n_d, now, sm, scale, (u32)dup);
        else launch_tun2_gather<W, true>(rs, d, pow_in, px0, reinterpret_cast<W*>(dig), n_d, now, sm, scale, (u32)dup);
        HIP_TRY(hipGetLastError());
        // constant term: crt of the E'-coefficients of c0 (evalLin itself is the inner product's starting value)
        if (px0 && (rc = crt_suffix<W>(rd, dup, x0, now * d, false, rs)) != ALCH_OK) return rc;
        // linear term: the digits' crt
        if ((rc = pow2_digit_tail<W>(rd, rs, x1, dig, now * d, GD, bw, b2first, b2kd)) != ALCH_OK) return rc;
        W* po = reinterpret_cast<W*>(reinterpret_cast<char*>(out) + done * 2 * ebs);
        const size_t pieces = (now + 3) / 4 * (size_t)L * (rs->n / Vec4<W>::LANES);
        const W* mx0 = c0_in_place ? reinterpret_cast<const W*>(src) : reinterpret_cast<const W*>(x0);
        const size_t x0_cts = c0_in_place ? 2 * (size_t)Lin * rr->n : (size_t)d * Lin * n_d;
        hipLaunchKernelGGL((k_tun2_mac<W, 4>), dim3(ew_grid(pieces)), dim3(256), 0, rs->stream, dev_ring<W>(rs), po, reinterpret_cast<const W*>(dig),
                           reinterpret_cast<const W*>(t->ks), now, d * GD, (u32)Lin, (!base2 && dup > 0) ? (u32)dup : 0u, t->sh, n_d, mx0, x0_cts,
                           reinterpret_cast<const W*>(t->lin), d, (u32)Lin, (u32)dup, sm, (c0_in_place && scale) ? 1 : 0);
        HIP_TRY(hipGetLastError());
    }
    return ALCH_OK;
}

extern "C" int alch_ct_tunnel(const alch_tunnel* t, const alch_buf* in, alch_buf* out, size_t batch, const uint64_t* s_pre, unsigned flags) try {
    if (!t || !in || !out) return fail(ALCH_E_INVALID, "null argument");
    if ((in->ring != t->rr && !is_suffix_ring(in->ring, t->rr)) || out->ring != t->rs)
        return fail(ALCH_E_INVALID, "input / output buffers must belong to the tunnel's rings (the input may live on the last limbs of the R' ring)");
    if (flags & ~(unsigned)(ALCH_POW_IN | ALCH_POW_OUT)) return fail(ALCH_E_INVALID, "unknown flag");
    if (batch == 0) return ALCH_OK;
    if (!pairs_ok(batch, in->n_elems) || !pairs_ok(batch, out->n_elems)) return fail(ALCH_E_INVALID, "buffers must hold 2*batch ring elements");
    // a tunnel from a ring to itself (R' = S', the key switch alone) has input and output on one ring: out may be a view into in
    if (bytes_overlap(out->dptr, 2 * batch * elem_bytes(out->ring), in->dptr, 2 * batch * elem_bytes(in->ring)))
        return fail(ALCH_E_INVALID, "alch_ct_tunnel: out must not alias the input");
    alch_ring* rs = t->rs;
    alch_ring* rr = t->rr;
    BIND(rs);
    alch_ring* rin = in->ring;
    int rc;
    if ((rc = ext_order(rs, rr, true)) != ALCH_OK) return rc;                       // everything runs on the target ring's stream
    if (rin != rr && (rc = ext_order(rs, rin, true)) != ALCH_OK) return rc;
    if (t->pow2) rc = ALCH_BY_WORD(rs, do_tunnel_pow2, t, rin, in->dptr, out->dptr, batch, s_pre, flags);
    else rc = ALCH_BY_WORD(rs, do_tunnel, t, rin, in->dptr, out->dptr, batch, s_pre, flags);
    if (rc != ALCH_OK) return rc;
    if (flags & ALCH_POW_OUT) if ((rc = buf_crt(out, 0, 2 * batch, true)) != ALCH_OK) return rc;
    if ((rc = ext_order(rs, rr, false)) != ALCH_OK) return rc;
    return rin != rr ? ext_order(rs, rin, false) : ALCH_OK;
} catch (...) { return abi_catch(); }

// ------------------------------------------------------------------------------------------------------
// Galois automorphisms sigma_j on the CRT basis (include/alchemy_hip.h, "Galois automorphisms"; automorph_host.hpp)
// ------------------------------------------------------------------------------------------------------
extern "C" int alch_automorph_table(uint32_t m, uint32_t j, uint32_t* out, size_t* len) try {
    if (!len) return fail(ALCH_E_INVALID, "null argument");
    automorph::Plan P;
    const int pc = automorph::plan(m, P);
    if (pc == automorph::PLAN_INVALID) return fail(ALCH_E_INVALID, "cyclotomic index must be >= 1");
    if (pc != automorph::PLAN_OK)
        return fail(ALCH_E_UNSUPPORTED, "alch_automorph_table: index " + std::to_string(m) + " is served on neither engine (odd primes <= 13, phi(m) <= 65535; two-power m <= 2^17)");
    if (automorph::gcd(j % m, m) != 1) return fail(ALCH_E_INVALID, "alch_automorph_table: j is not a unit mod m");
    if (!out) { *len = P.n; return ALCH_OK; }
    if (*len < P.n) return fail(ALCH_E_INVALID, "alch_automorph_table: capacity below phi(m)");
    std::vector<uint32_t> t;
    automorph::build_table(P, j, t);
    memcpy(out, t.data(), t.size() * sizeof(uint32_t));
    *len = P.n;
    return ALCH_OK;
} catch (...) { return abi_catch(); }

// General engine: the device table of sigma_j (j reduced mod m, a unit), cached in the ring.  At most AUTOTAB_MAX tables stay; the
// oldest leaves after the stream has drained (a queued gather may still read it).
constexpr size_t AUTOTAB_MAX = 64;
static int automorph_dev_table(alch_ring* r, u32 j, const u32** out) {
    ALCH_REQUIRE_DEVICE_LOCK(r, "automorph_dev_table");
    for (auto& e : r->autotab) if (e.first == j) { *out = e.second; return ALCH_OK; }
    automorph::Plan P;
    std::vector<uint32_t> t;
    if (automorph::plan(r->m, P) != automorph::PLAN_OK || P.n != r->n || !automorph::build_table(P, j, t))
        return fail(ALCH_E_INTERNAL, "automorphism table: the ring's index has no plan");
    if (r->autotab.size() >= AUTOTAB_MAX) {
        HIP_TRY(hipStreamSynchronize(r->stream));
        (void)hipFree(r->autotab.front().second);
        r->autotab.pop_front();
    }
    u32* d = nullptr;
    if (hipMalloc((void**)&d, t.size() * sizeof(u32)) != hipSuccess) return fail(ALCH_E_NOMEM, "hipMalloc(automorphism table) failed");
    if (hipMemcpy(d, t.data(), t.size() * sizeof(u32), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        return fail(ALCH_E_HIP, "automorphism table upload failed");
    }
    r->autotab.emplace_back(j, d);
    *out = d;
    return ALCH_OK;
}

// dst[e] = sigma_j(src[e]), e < count, CRT basis; dst and src share no byte (the callers check).  tab: general engine only.
template <typename W>
static int launch_automorph(alch_ring* r, void* dst, const void* src, size_t count, u32 j, const u32* tab) {
    constexpr int VL = Vec4<W>::LANES;
    const size_t words = count * elem_words(r);
    if (!r->gen)                                   // n >= 16: a multiple of the vector width
        hipLaunchKernelGGL((k_automorph_pow2<W, VL>), dim3(ew_grid(words / VL)), dim3(256), 0, r->stream, dev_ring<W>(r), (W*)dst, (const W*)src, words, j, r->logn);
    else if (r->n % VL == 0)
        hipLaunchKernelGGL((k_automorph_tab<W, VL>), dim3(ew_grid(words / VL)), dim3(256), 0, r->stream, dev_ring<W>(r), (W*)dst, (const W*)src, words, tab);
    else
        hipLaunchKernelGGL((k_automorph_tab<W, 1>), dim3(ew_grid(words)), dim3(256), 0, r->stream, dev_ring<W>(r), (W*)dst, (const W*)src, words, tab);
    HIP_TRY(hipGetLastError());
    return ALCH_OK;
}

extern "C" int alch_buf_automorph(alch_buf* dst, size_t dst_first, const alch_buf* src, size_t src_first, size_t count, uint32_t j) try {
    if (!dst || !src) return fail(ALCH_E_INVALID, "null buffer");
    if (dst->ring != src->ring) return fail(ALCH_E_INVALID, "buffers belong to different rings");
    if (!range_ok(dst_first, count, dst->n_elems) || !range_ok(src_first, count, src->n_elems)) return fail(ALCH_E_INVALID, "element range out of bounds");
    alch_ring* r = dst->ring;
    if (!r->has_crt) return fail(ALCH_E_NO_CRT, "this ring has no CRT basis (created with alch_ring_create_nocrt)");
    j %= r->m;
    if (automorph::gcd(j, r->m) != 1) return fail(ALCH_E_INVALID, "alch_buf_automorph: j is not a unit mod m");
    if (count == 0) return ALCH_OK;
    BIND(r);
    char* d = reinterpret_cast<char*>(dst->dptr) + dst_first * elem_bytes(r);
    const char* f = reinterpret_cast<const char*>(src->dptr) + src_first * elem_bytes(r);
    if (bytes_overlap(d, count * elem_bytes(r), f, count * elem_bytes(r)))
        return fail(ALCH_E_INVALID, "alch_buf_automorph: the written range overlaps the read range (a gather cannot run in place)");
    const u32* tab = nullptr;
    int rc;
    if (r->gen && (rc = automorph_dev_table(r, j, &tab)) != ALCH_OK) return rc;
    return ALCH_BY_WORD(r, launch_automorph, r, d, f, count, j, tab);
} catch (...) { return abi_catch(); }

// sigma_j on linear ciphertexts at one key switch: the gather into the ring's scratch, then the ring-to-itself tunnel stage with
// lin = crt(1) and d_rel = 1 -- out = (s_pre sigma_j(c0), 0) + switch(hint, s_pre sigma_j(c1)) -- on the permuted chunk.  The
// tunnel kernels are the ones alch_ct_tunnel runs, so the words are those of alch_buf_automorph followed by alch_ct_tunnel.
struct alch_automorph {
    alch_ring* ring;
    u32 j;                                     // reduced mod m
    alch_tunnel* tun;                          // ring -> ring, lin = crt(1), the caller's hint (owned)
};

extern "C" int alch_automorph_create(alch_ring* ring, uint32_t j, int gadget, const alch_buf* ks_crt, void** out) try {
    if (!ring || !ks_crt || !out) return fail(ALCH_E_INVALID, "null argument");
    *out = nullptr;
    if (gadget_width(gadget) < 0) return fail(ALCH_E_INVALID, "alch_automorph_create: unknown gadget");
    if (ks_crt->ring != ring) return fail(ALCH_E_INVALID, "alch_automorph_create: the hint lives in the ring");
    if (!ring->has_crt) return fail(ALCH_E_NO_CRT, "this ring has no CRT basis (created with alch_ring_create_nocrt)");
    j %= ring->m;
    if (automorph::gcd(j, ring->m) != 1) return fail(ALCH_E_INVALID, "alch_automorph_create: j is not a unit mod m");
    if (ks_crt->n_elems < 2 * (size_t)gadget_digits(ring, gadget)) return fail(ALCH_E_INVALID, "alch_automorph_create: need 2 * (gadget digits) hint elements");
    BIND(ring);
    int rc;
    const u32* tab = nullptr;
    if (ring->gen && (rc = automorph_dev_table(ring, j, &tab)) != ALCH_OK) return rc;
    alch_buf* one = nullptr;                   // crt(1): the constant 1 in every slot of every limb
    if ((rc = alch_buf_alloc(ring, 1, &one)) != ALCH_OK) return rc;
    std::vector<int64_t> ones(elem_words(ring), 1);
    alch_tunnel* t = nullptr;
    if ((rc = alch_buf_upload(one, 0, 1, ones.data())) == ALCH_OK) rc = alch_tunnel_create(ring, ring, gadget, one, ks_crt, &t);
    const std::string msg = g_err;             // alch_tunnel_create has drained the stream: `one` and `ones` are no longer read
    alch_buf_free(one);
    if (rc != ALCH_OK) return fail(rc, msg);
    *out = new alch_automorph{ring, j, t};
    return ALCH_OK;
} catch (...) { return abi_catch(); }

extern "C" int alch_automorph_free(void* handle) try {
    alch_automorph* a = reinterpret_cast<alch_automorph*>(handle);
    if (!a) return ALCH_OK;
    alch_tunnel_free(a->tun);
    delete a;
    return ALCH_OK;
} catch (...) { return abi_catch(); }

extern "C" int alch_ct_automorph(const void* handle, const alch_buf* in, alch_buf* out, size_t batch, const uint64_t* s_pre, unsigned flags) try {
    const alch_automorph* a = reinterpret_cast<const alch_automorph*>(handle);
    if (!a || !in || !out) return fail(ALCH_E_INVALID, "null argument");
    alch_ring* r = a->ring;
    if (in->ring != r || out->ring != r) return fail(ALCH_E_INVALID, "alch_ct_automorph: input and output buffers belong to the automorphism's ring");
    if (flags & ~(unsigned)(ALCH_POW_IN | ALCH_POW_OUT)) return fail(ALCH_E_INVALID, "unknown flag");
    if (flags) return fail(ALCH_E_UNSUPPORTED, "alch_ct_automorph: CRT basis in and out only (on the powerful basis sigma_j is not a permutation: transform first)");
    if (batch == 0) return ALCH_OK;
    if (!pairs_ok(batch, in->n_elems) || !pairs_ok(batch, out->n_elems)) return fail(ALCH_E_INVALID, "buffers must hold 2*batch ring elements");
    const size_t eb = elem_bytes(r);
    if (bytes_overlap(out->dptr, 2 * batch * eb, in->dptr, 2 * batch * eb)) return fail(ALCH_E_INVALID, "alch_ct_automorph: out must not alias the input");
    BIND(r);
    int rc;
    const u32* tab = nullptr;
    if (r->gen && (rc = automorph_dev_table(r, a->j, &tab)) != ALCH_OK) return rc;
    const size_t chunk = scratch_chunk(r->scratch_mib << 20, batch, 2 * eb);
    if ((rc = r->ws_auto.reserve(chunk * 2 * eb)) != ALCH_OK) return rc;
    for (size_t done = 0; done < batch; done += chunk) {
        const size_t now = std::min(chunk, batch - done);
        const char* src = reinterpret_cast<const char*>(in->dptr) + done * 2 * eb;
        char* dst = reinterpret_cast<char*>(out->dptr) + done * 2 * eb;
        if ((rc = ALCH_BY_WORD(r, launch_automorph, r, r->ws_auto.p, src, 2 * now, a->j, tab)) != ALCH_OK) return rc;
        if (a->tun->pow2) rc = ALCH_BY_WORD(r, do_tunnel_pow2, a->tun, r, r->ws_auto.p, dst, now, s_pre, 0u);
        else rc = ALCH_BY_WORD(r, do_tunnel, a->tun, r, r->ws_auto.p, dst, now, s_pre, 0u);
        if (rc != ALCH_OK) return rc;
    }
    return ALCH_OK;
} catch (...) { return abi_catch(); }

// ------------------------------------------------------------------------------------------------------
// Hoisted automorphisms (include/alchemy_hip.h, "Hoisted automorphisms"; kernel_hoist.hpp)
// ------------------------------------------------------------------------------------------------------
// Several sigma_j of one batch at one decomposition: the digits of s_pre c1 are brought to CRT form exactly as the ring-to-itself
// tunnel's composed path brings them (do_tunnel_pow2 / do_tunnel with d_rel = 1, lin = crt(1); never the fused TrivGad kernels, which
// keep no digits), then every rotation reads them through its slot permutation inside the hint inner product.
struct alch_automorph_set {
    alch_ring* ring;
    int gadget, digits;                        // gadget code; D = its digit count on the ring
    u32 n_j;
    u32 j[HOIST_MAX];                          // reduced mod m
    void* ks;                                  // the n_j hints one after the other, 2 D elements each, Montgomery form (owned)
    u32* tabs;                                 // general engine: [n_j][n] slot tables (owned: the ring's cache may evict its own)
    int32_t* ident;                            // general engine: the coefficient table of the tunnel from the ring to itself, k -> k
};

extern "C" int alch_automorph_set_free(void* handle) try {
    alch_automorph_set* a = reinterpret_cast<alch_automorph_set*>(handle);
    if (!a) return ALCH_OK;
    (void)hipSetDevice(a->ring->device);
    (void)hipStreamSynchronize(a->ring->stream);
    if (a->ks) (void)hipFree(a->ks);
    if (a->tabs) (void)hipFree(a->tabs);
    if (a->ident) (void)hipFree(a->ident);
    delete a;
    return ALCH_OK;
} catch (...) { return abi_catch(); }

extern "C" int alch_automorph_set_create(alch_ring* ring, uint32_t n_j, const uint32_t* j, int gadget, const alch_buf* ks_crt, void** out) try {
    if (!ring || !j || !ks_crt || !out) return fail(ALCH_E_INVALID, "alch_automorph_set_create: null argument");
    *out = nullptr;
    if (gadget_width(gadget) < 0) return fail(ALCH_E_INVALID, "alch_automorph_set_create: unknown gadget");
    if (ks_crt->ring != ring) return fail(ALCH_E_INVALID, "alch_automorph_set_create: the hints live in the ring");
    if (!ring->has_crt) return fail(ALCH_E_NO_CRT, "this ring has no CRT basis (created with alch_ring_create_nocrt)");
    if (n_j < 1 || n_j > (uint32_t)HOIST_MAX)
        return fail(ALCH_E_INVALID, "alch_automorph_set_create: a set holds 1 .. " + std::to_string(HOIST_MAX) + " units");
    for (u32 r = 0; r < n_j; ++r)
        if (automorph::gcd(j[r] % ring->m, ring->m) != 1)
            return fail(ALCH_E_INVALID, "alch_automorph_set_create: j[" + std::to_string(r) + "] is not a unit mod m");
    const int D = gadget_digits(ring, gadget);
    const size_t nks = (size_t)n_j * 2 * (size_t)D;
    if (ks_crt->n_elems < nks) return fail(ALCH_E_INVALID, "alch_automorph_set_create: need n_j * 2 * (gadget digits) hint elements");
    BIND(ring);
    alch_automorph_set* a = new alch_automorph_set{ring, gadget, D, n_j, {0}, nullptr, nullptr, nullptr};
    for (u32 r = 0; r < n_j; ++r) a->j[r] = j[r] % ring->m;
    if (hipMalloc(&a->ks, nks * elem_bytes(ring)) != hipSuccess) {
        alch_automorph_set_free(a);
        return fail(ALCH_E_NOMEM, "alch_automorph_set_create: hipMalloc(hints) failed");
    }
    if (ring->gen) {
        automorph::Plan P;
        if (automorph::plan(ring->m, P) != automorph::PLAN_OK || P.n != ring->n) {
            alch_automorph_set_free(a);
            return fail(ALCH_E_INTERNAL, "alch_automorph_set_create: the ring's index has no plan");
        }
        const size_t n = ring->n;
        std::vector<uint32_t> all(n_j * n), t;
        for (u32 r = 0; r < n_j; ++r) {
            automorph::build_table(P, a->j[r], t);
            std::copy(t.begin(), t.end(), all.begin() + r * n);
        }
        std::vector<int32_t> id(n);
        for (size_t k = 0; k < n; ++k) id[k] = (int32_t)k;
        if (hipMalloc((void**)&a->tabs, all.size() * sizeof(u32)) != hipSuccess || hipMalloc((void**)&a->ident, n * sizeof(int32_t)) != hipSuccess) {
            alch_automorph_set_free(a);
            return fail(ALCH_E_NOMEM, "alch_automorph_set_create: hipMalloc(tables) failed");
        }
        if (hipMemcpy(a->tabs, all.data(), all.size() * sizeof(u32), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(a->ident, id.data(), n * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
            alch_automorph_set_free(a);
            return fail(ALCH_E_HIP, "alch_automorph_set_create: table upload failed");
        }
    }
    int rc = ALCH_BY_WORD(ring, tunnel_to_mont, ring, a->ks, ks_crt->dptr, nks);
    if (rc != ALCH_OK) { const std::string msg = g_err; alch_automorph_set_free(a); return fail(rc, msg); }
    if (hipStreamSynchronize(ring->stream) != hipSuccess) { alch_automorph_set_free(a); return fail(ALCH_E_HIP, "alch_automorph_set_create: setup failed"); }
    *out = a;
    return ALCH_OK;
} catch (...) { return abi_catch(); }

// rotations r0 .. r0 + nrot - 1 of the set, accumulated into the `now` ciphertexts at po (kernel_hoist.hpp)
template <typename W>
static void launch_hoist_mac(alch_ring* r, W* po, const W* dig, const W* cin, size_t now, u32 D, const HoistSet<W>& S, u32 r0, u32 nrot,
                             const Scal<W>& sm, bool scale) {
    constexpr int VL = Vec4<W>::LANES;
    const size_t tiles = (now + 3) / 4 * (size_t)r->L;
    const int sc = scale ? 1 : 0;
    if (!r->gen)                                   // n >= 16: a multiple of the vector width
        hipLaunchKernelGGL((k_hoist_mac<W, VL, 4, true>), dim3(ew_grid(tiles * (r->n / VL))), dim3(256), 0, r->stream, dev_ring<W>(r), po, dig, cin, now, D, S,
                           r0, nrot, r->logn, sm, sc);
    else if (r->n % VL == 0)
        hipLaunchKernelGGL((k_hoist_mac<W, VL, 4, false>), dim3(ew_grid(tiles * (r->n / VL))), dim3(256), 0, r->stream, dev_ring<W>(r), po, dig, cin, now, D, S,
                           r0, nrot, 0, sm, sc);
    else
        hipLaunchKernelGGL((k_hoist_mac<W, 1, 4, false>), dim3(ew_grid(tiles * r->n)), dim3(256), 0, r->stream, dev_ring<W>(r), po, dig, cin, now, D, S,
                           r0, nrot, 0, sm, sc);
}

// The walk both hoisted calls share: per chunk of at most "scratch_mib", the digits of s_pre c1 in CRT form, then
// body(done, now, GD, digits, cin, S, sm, scale) queues the inner products over the GD digits of the chunk's `now` ciphertexts from
// ciphertext `done` on.
template <typename W, typename Body>
static int hoist_walk(const alch_automorph_set* a, const void* in, size_t batch, const uint64_t* s_pre, Body body) {
    alch_ring* r = a->ring;
    const int L = r->L;
    const u32 bw = (u32)gadget_width(a->gadget);      // BaseBGad 2^bw; 0: TrivGad
    const bool base2 = bw > 0;
    const u32 GD = base2 ? (u32)a->digits : (u32)L;
    Scal<u32> b2first, b2kd;
    if (base2) base2_layout(r, b2first, b2kd, bw);
    const size_t eb = elem_bytes(r), ew = elem_words(r);
    // scratch per ciphertext: the Pow copy of the input (2 elements); the scaled c1 where a decomposition reads it (general engine:
    // k_tunnel_gather writes the scaled c0 next to it); the GD digit elements
    const size_t x0_b = r->gen ? eb : 0, x1_b = (r->gen || base2) ? eb : 0, dig_b = (size_t)GD * eb;
    const size_t per_ct = 2 * eb + x0_b + x1_b + dig_b;
    const size_t chunk = scratch_chunk(r->scratch_mib << 20, batch, per_ct);
    int rc = r->ws_full.reserve(chunk * per_ct);
    if (rc != ALCH_OK) return rc;
    Carve cv(r->ws_full.p, chunk);
    char *win = cv.take(2 * eb), *x0 = cv.take(x0_b), *x1 = cv.take(x1_b), *dig = cv.take(dig_b);
    if (!cv.matches(per_ct)) return fail(ALCH_E_INTERNAL, "hoist_walk: the scratch carve differs from the bytes reserved per ciphertext");
    uint64_t s_eff[MAXL] = {0};
    for (int i = 0; i < L; ++i) s_eff[i] = up_scalar(r, 0, i, s_pre ? s_pre[i] : 1);
    const bool scale = s_pre != nullptr;
    Scal<W> sm;
    scal_to_mont<W>(r, s_eff, 1, sm);
    HoistSet<W> S{};
    for (u32 t = 0; t < a->n_j; ++t) {
        S.hint[t] = reinterpret_cast<const W*>(a->ks) + (size_t)t * 2 * GD * ew;
        S.tab[t] = a->tabs ? a->tabs + (size_t)t * r->n : nullptr;
        S.j[t] = a->j[t];
    }
    for (size_t done = 0; done < batch; done += chunk) {
        const size_t now = std::min(chunk, batch - done);
        const char* src = reinterpret_cast<const char*>(in) + done * 2 * eb;
        if (!r->gen) {                                 // do_tunnel_pow2 with d = 1, up to its inner product
            if ((rc = crt_into<W>(r, win, {src}, 2 * now, true, r)) != ALCH_OK) return rc;
            const W* pow_in = reinterpret_cast<const W*>(win);
            if (base2) launch_tun2_gather<W, false>(r, 1, pow_in, nullptr, reinterpret_cast<W*>(x1), r->n, now, sm, scale, 0u);
            else launch_tun2_gather<W, true>(r, 1, pow_in, nullptr, reinterpret_cast<W*>(dig), r->n, now, sm, scale, 0u);
            HIP_TRY(hipGetLastError());
            if ((rc = pow2_digit_tail<W>(r, r, x1, dig, now, GD, bw, b2first, b2kd)) != ALCH_OK) return rc;
        } else {                                       // do_tunnel with d_rel = 1, rx = the ring, up to its inner product
            if ((rc = do_crt<W>(r, win, 0, 2 * now, true, src, r)) != ALCH_OK) return rc;
            const size_t gw = now * 2 * ew;
            ALCH_LAUNCH_VW(k_tunnel_gather, r, gw, r->stream, dev_ring<W>(r), (const W*)win, (const W*)win, (W*)x0, (W*)x1, a->ident, 1u, r->n, now, sm,
                           scale ? 1 : 0, (u32)L, 0u, 0u);
            HIP_TRY(hipGetLastError());
            if ((rc = gen_digit_tail<W>(r, r, x1, dig, now, GD, (u32)L, 0u, bw, b2first, b2kd)) != ALCH_OK) return rc;
        }
        if ((rc = body(done, now, GD, reinterpret_cast<const W*>(dig), reinterpret_cast<const W*>(src), S, sm, scale)) != ALCH_OK) return rc;
    }
    return ALCH_OK;
}

template <typename W>
static int do_hoisted(const alch_automorph_set* a, const void* in, void* out, size_t batch, const uint64_t* s_pre, bool sum) {
    alch_ring* r = a->ring;
    const size_t eb = elem_bytes(r);
    return hoist_walk<W>(a, in, batch, s_pre, [&](size_t done, size_t now, u32 GD, const W* pd, const W* cin, const HoistSet<W>& S, const Scal<W>& sm, bool scale) -> int {
        if (sum) {
            launch_hoist_mac<W>(r, reinterpret_cast<W*>(reinterpret_cast<char*>(out) + done * 2 * eb), pd, cin, now, GD, S, 0u, a->n_j, sm, scale);
            HIP_TRY(hipGetLastError());
        } else {
            for (u32 t = 0; t < a->n_j; ++t) {
                launch_hoist_mac<W>(r, reinterpret_cast<W*>(reinterpret_cast<char*>(out) + ((size_t)t * batch + done) * 2 * eb), pd, cin, now, GD, S, t, 1u,
                                    sm, scale);
                HIP_TRY(hipGetLastError());
            }
        }
        return ALCH_OK;
    });
}

extern "C" int alch_ct_automorph_hoisted(const void* handle, const alch_buf* in, alch_buf* out, size_t batch, const uint64_t* s_pre, unsigned flags) try {
    const alch_automorph_set* a = reinterpret_cast<const alch_automorph_set*>(handle);
    if (!a || !in || !out) return fail(ALCH_E_INVALID, "alch_ct_automorph_hoisted: null argument");
    alch_ring* r = a->ring;
    if (in->ring != r || out->ring != r) return fail(ALCH_E_INVALID, "alch_ct_automorph_hoisted: input and output buffers belong to the set's ring");
    if (flags & ~(unsigned)(ALCH_POW_IN | ALCH_POW_OUT | ALCH_AUTO_SUM)) return fail(ALCH_E_INVALID, "alch_ct_automorph_hoisted: unknown flag");
    if (flags & (ALCH_POW_IN | ALCH_POW_OUT))
        return fail(ALCH_E_UNSUPPORTED, "alch_ct_automorph_hoisted: CRT basis in and out only (on the powerful basis sigma_j is not a permutation: transform first)");
    if (batch == 0) return ALCH_OK;
    const bool sum = (flags & ALCH_AUTO_SUM) != 0;
    const size_t rots = sum ? 1 : (size_t)a->n_j;
    if (!pairs_ok(batch, in->n_elems) || batch > out->n_elems / 2 / rots)
        return fail(ALCH_E_INVALID, "alch_ct_automorph_hoisted: in holds 2 * batch elements, out 2 * n_j * batch (2 * batch with ALCH_AUTO_SUM)");
    const size_t eb = elem_bytes(r);
    if (bytes_overlap(out->dptr, 2 * rots * batch * eb, in->dptr, 2 * batch * eb)) return fail(ALCH_E_INVALID, "alch_ct_automorph_hoisted: out must not alias the input");
    BIND(r);
    return ALCH_BY_WORD(r, do_hoisted, a, in->dptr, out->dptr, batch, s_pre, sum);
} catch (...) { return abi_catch(); }

// ------------------------------------------------------------------------------------------------------
// Weighted sums of hoisted rotations (include/alchemy_hip.h, "Weighted sums of hoisted rotations"; kernel_lincomb.hpp)
// ------------------------------------------------------------------------------------------------------
// rows [0, nrows) of one row block over the chunk's `now` ciphertexts: the forms and the dispatch of launch_hoist_mac
template <typename W>
static void launch_hoist_lincomb(alch_ring* r, W* po, const W* dig, const W* cin, size_t now, u32 D, const HoistSet<W>& S, u32 nrot, const Scal<W>& sm,
                                 bool scale, const W* wts, u32 nrows, size_t ostride) {
    constexpr int VL = Vec4<W>::LANES, TL = LINCOMB_TILE, RW = LINCOMB_ROWS;
    const size_t tiles = (now + TL - 1) / TL * (size_t)r->L;
    const int sc = scale ? 1 : 0;
    if (!r->gen)                                   // n >= 16: a multiple of the vector width
        hipLaunchKernelGGL((k_hoist_lincomb<W, VL, TL, true, RW>), dim3(ew_grid(tiles * (r->n / VL))), dim3(256), 0, r->stream, dev_ring<W>(r), po, dig, cin,
                           now, D, S, nrot, r->logn, sm, sc, wts, nrows, ostride);
    else if (r->n % VL == 0)
        hipLaunchKernelGGL((k_hoist_lincomb<W, VL, TL, false, RW>), dim3(ew_grid(tiles * (r->n / VL))), dim3(256), 0, r->stream, dev_ring<W>(r), po, dig, cin,
                           now, D, S, nrot, 0, sm, sc, wts, nrows, ostride);
    else
        hipLaunchKernelGGL((k_hoist_lincomb<W, 1, TL, false, RW>), dim3(ew_grid(tiles * r->n)), dim3(256), 0, r->stream, dev_ring<W>(r), po, dig, cin, now, D,
                           S, nrot, 0, sm, sc, wts, nrows, ostride);
}

template <typename W>
static int do_lincomb(const alch_automorph_set* a, const void* wts, size_t n_out, const void* in, void* out, size_t batch, const uint64_t* s_pre) {
    alch_ring* r = a->ring;
    const size_t ew = elem_words(r);
    const size_t nblk = lincomb_blocks(n_out, LINCOMB_ROWS);
    return hoist_walk<W>(a, in, batch, s_pre, [&](size_t done, size_t now, u32 GD, const W* pd, const W* cin, const HoistSet<W>& S, const Scal<W>& sm, bool scale) -> int {
        for (size_t i = 0; i < nblk; ++i) {
            const size_t g0 = i * LINCOMB_ROWS;
            launch_hoist_lincomb<W>(r, reinterpret_cast<W*>(out) + (g0 * batch + done) * 2 * ew, pd, cin, now, GD, S, a->n_j, sm, scale,
                                    reinterpret_cast<const W*>(wts) + g0 * a->n_j * ew, (u32)lincomb_block_rows(n_out, LINCOMB_ROWS, i), batch * 2 * ew);
            HIP_TRY(hipGetLastError());
        }
        return ALCH_OK;
    });
}

extern "C" int alch_ct_automorph_lincomb(const void* handle, const alch_buf* w_crt, size_t w_first, size_t n_out, const alch_buf* in, alch_buf* out,
                                         size_t batch, const uint64_t* s_pre, unsigned flags) try {
    const alch_automorph_set* a = reinterpret_cast<const alch_automorph_set*>(handle);
    if (!a || !w_crt || !in || !out) return fail(ALCH_E_INVALID, "alch_ct_automorph_lincomb: null argument");
    alch_ring* r = a->ring;
    if (w_crt->ring != r || in->ring != r || out->ring != r)
        return fail(ALCH_E_INVALID, "alch_ct_automorph_lincomb: the weights, the input and the output belong to the set's ring");
    if (flags & ~(unsigned)(ALCH_POW_IN | ALCH_POW_OUT)) return fail(ALCH_E_INVALID, "alch_ct_automorph_lincomb: unknown flag");
    if (flags)
        return fail(ALCH_E_UNSUPPORTED, "alch_ct_automorph_lincomb: CRT basis in and out only (on the powerful basis sigma_j is not a permutation: transform first)");
    if (batch == 0 || n_out == 0) return ALCH_OK;
    const size_t R = a->n_j;
    if (n_out > w_crt->n_elems / R || !range_ok(w_first, n_out * R, w_crt->n_elems))
        return fail(ALCH_E_INVALID, "alch_ct_automorph_lincomb: w_crt holds n_out * n_j elements from w_first on");
    if (!pairs_ok(batch, in->n_elems) || batch > out->n_elems / 2 / n_out)
        return fail(ALCH_E_INVALID, "alch_ct_automorph_lincomb: in holds 2 * batch elements, out 2 * n_out * batch");
    const size_t eb = elem_bytes(r);
    const char* wp = reinterpret_cast<const char*>(w_crt->dptr) + w_first * eb;
    if (bytes_overlap(out->dptr, 2 * n_out * batch * eb, in->dptr, 2 * batch * eb)) return fail(ALCH_E_INVALID, "alch_ct_automorph_lincomb: out must not alias the input");
    if (bytes_overlap(out->dptr, 2 * n_out * batch * eb, wp, n_out * R * eb)) return fail(ALCH_E_INVALID, "alch_ct_automorph_lincomb: out must not alias the weights");
    BIND(r);
    return ALCH_BY_WORD(r, do_lincomb, a, wp, n_out, in->dptr, out->dptr, batch, s_pre);
} catch (...) { return abi_catch(); }

// ------------------------------------------------------------------------------------------------------
// SymmSHE modSwitch on batches of linear ciphertexts (Eval.hs:130; PT2CT.hs:177,224-229)
// ------------------------------------------------------------------------------------------------------
// per = 2: linear ciphertexts (c0 rescaled on the decoding basis, c1 on the powerful basis); per = 3: quadratic ciphertexts (c0, c1, c2),
// c2 on the powerful basis like c1 (alch_ct_mod_switch_deg); per = 1: `batch` single ring elements, all on
// the powerful basis (the c2 of a quadratic ciphertext: SymmSHE's modSwitch rescales every coefficient above c0 with rescalePow)
template <typename W>
static int do_mod_switch(alch_ring* rin, alch_ring* rout, const void* in, void* out, size_t batch, unsigned flags, int per) {
    const size_t n = rin->n;
    const size_t P = (size_t)per;
    if (rout->L > rin->L) {                                   // up: Rescale b -> (a, b), any basis
        const int dup = rout->L - rin->L;
        uint64_t mult[MAXL] = {0};
        for (int j = dup; j < rout->L; ++j) mult[j] = up_scalar(rout, dup, j, 1);
        Scal<W> sm;
        scal_to_mont<W>(rout, mult, 1, sm);
        const size_t total = P * batch * elem_words(rout);
        hipLaunchKernelGGL((k_rescale_up<W>), dim3(ew_grid(total)), dim3(256), 0, rout->stream, dev_ring<W>(rout), (const W*)in, (W*)out,
                           P * batch, dup, sm);
        HIP_TRY(hipGetLastError());
        return ALCH_OK;
    }
    // down: Pow basis (c0 on the Dec basis for a general index), one limb at a time, outermost first
    const int L = rin->L, ddn = L - rout->L;
    const size_t eb = elem_bytes(rin);
    const bool dec_c0 = per >= 2 && rin->gen && rin->gh.rad > 1;
    if (rin->gen && rin->opts.rs_lin && ddn <= MAXDROP && !(flags & ALCH_POW_IN)) {
        // kept limbs stay in the CRT basis
        const size_t per_b = P * (size_t)ddn * n * sizeof(W);
        const size_t chunk = scratch_chunk(rin->scratch_mib << 20, batch, per_b);
        int rc = rin->ws_full.reserve(chunk * per_b);
        if (rc != ALCH_OK) return rc;
        for (size_t done = 0; done < batch; done += chunk) {
            const size_t now = std::min(chunk, batch - done);
            if ((rc = rescale_down_crt<W>(rin, ddn, reinterpret_cast<const char*>(in) + done * P * eb, rin->ws_full.p,
                                          reinterpret_cast<char*>(out) + done * P * elem_bytes(rout), P * now, dec_c0,
                                          (flags & ALCH_POW_OUT) != 0, P)) != ALCH_OK) return rc;
        }
        return ALCH_OK;
    }
    const size_t per_ct = 3 * P * eb;                          // Pow copy + ping + pong
    const size_t chunk = scratch_chunk(rin->scratch_mib << 20, batch, per_ct);
    int rc = rin->ws_full.reserve(chunk * per_ct);
    if (rc != ALCH_OK) return rc;
    Carve cv(rin->ws_full.p, chunk);
    char *cur0 = cv.take(P * eb), *ping = cv.take(P * eb), *pong = cv.take(P * eb);
    if (!cv.matches(per_ct)) return fail(ALCH_E_INTERNAL, "do_mod_switch: the scratch carve differs from the bytes reserved per ciphertext");
    const size_t in_bytes = P * eb;
    for (size_t done = 0; done < batch; done += chunk) {
        const size_t now = std::min(chunk, batch - done);
        const char* src = reinterpret_cast<const char*>(in) + done * in_bytes;
        if (flags & ALCH_POW_IN) HIP_TRY(hipMemcpyAsync(cur0, src, now * in_bytes, hipMemcpyDeviceToDevice, rin->stream));
        else if ((rc = crt_into<W>(rin, cur0, {src}, P * now, true)) != ALCH_OK) return rc;
        if ((rc = rescale_down_limbs<W>(rin, rout, cur0, ping, pong, out, done, now, P, dec_c0, (flags & ALCH_POW_OUT) != 0)) != ALCH_OK) return rc;
    }
    return ALCH_OK;
}

extern "C" int alch_ct_mod_switch(const alch_buf* in, alch_buf* out, size_t batch, unsigned flags) try {
    if (!in || !out) return fail(ALCH_E_INVALID, "null buffer");
    alch_ring* rin = in->ring;
    alch_ring* rout = out->ring;
    if (flags & ~(unsigned)(ALCH_POW_IN | ALCH_POW_OUT)) return fail(ALCH_E_INVALID, "unknown flag");
    if (!rin->has_crt || !rout->has_crt) return fail(ALCH_E_NO_CRT, "modSwitch runs on rings with a CRT basis");
    const bool up = rout->L > rin->L;
    if (rin->L == rout->L || !(up ? is_suffix_ring(rin, rout) : is_suffix_ring(rout, rin)))
        return fail(ALCH_E_INVALID, "the smaller ring's moduli must be the last limbs of the bigger ring's (same index and word size)");
    // no overlap check: rin->L != rout->L, so in and out belong to two rings, a view keeps its parent's ring and two allocations share no byte
    if (batch == 0) return ALCH_OK;
    if (!pairs_ok(batch, in->n_elems) || !pairs_ok(batch, out->n_elems)) return fail(ALCH_E_INVALID, "buffers must hold 2*batch ring elements");
    alch_ring* rw = up ? rout : rin;                          // the ring whose stream carries the work
    alch_ring* ro = up ? rin : rout;
    BIND(rw);
    int rc;
    if ((rc = ext_order(rw, ro, true)) != ALCH_OK) return rc;
    if ((rc = ALCH_BY_WORD(rin, do_mod_switch, rin, rout, in->dptr, out->dptr, batch, flags)) != ALCH_OK) return rc;
    return ext_order(rw, ro, false);
} catch (...) { return abi_catch(); }

// The same for ciphertexts of degree 1 or 2 (within ABI 1.8): degree 1 is alch_ct_mod_switch word for word, degree 2 switches the
// quadratic ciphertext between (*) and keySwitchQuadCirc (PT2CT.hs:177 inner modSwitch_), c0 on the decoding basis, c1 and c2 on the powerful.
extern "C" int alch_ct_mod_switch_deg(const alch_buf* in, alch_buf* out, size_t batch, int degree, unsigned flags) try {
    if (!in || !out) return fail(ALCH_E_INVALID, "alch_ct_mod_switch_deg: null buffer");
    alch_ring* rin = in->ring;
    alch_ring* rout = out->ring;
    if (flags & ~(unsigned)(ALCH_POW_IN | ALCH_POW_OUT)) return fail(ALCH_E_INVALID, "alch_ct_mod_switch_deg: unknown flag");
    if (degree != 1 && degree != 2) return fail(ALCH_E_INVALID, "alch_ct_mod_switch_deg: degree must be 1 or 2");
    const bool up = rout->L > rin->L;
    if (rin->L == rout->L || !(up ? is_suffix_ring(rin, rout) : is_suffix_ring(rout, rin)))
        return fail(ALCH_E_INVALID, "alch_ct_mod_switch_deg: the smaller ring's moduli must be the last limbs of the bigger ring's (same index and word size)");
    const size_t per = (size_t)degree + 1;
    if (batch > in->n_elems / per || batch > out->n_elems / per)
        return fail(ALCH_E_INVALID, "alch_ct_mod_switch_deg: buffers must hold (degree + 1) * batch ring elements");
    if (!rin->has_crt || !rout->has_crt) return fail(ALCH_E_NO_CRT, "alch_ct_mod_switch_deg: modSwitch runs on rings with a CRT basis");
    // no overlap check: the limb counts differ, so in and out belong to two rings and to two allocations (see alch_ct_mod_switch)
    if (batch == 0) return ALCH_OK;
    alch_ring* rw = up ? rout : rin;                          // the ring whose stream carries the work
    alch_ring* ro = up ? rin : rout;
    BIND(rw);
    int rc;
    if ((rc = ext_order(rw, ro, true)) != ALCH_OK) return rc;
    if ((rc = ALCH_BY_WORD(rin, do_mod_switch, rin, rout, in->dptr, out->dptr, batch, flags, (int)per)) != ALCH_OK) return rc;
    return ext_order(rw, ro, false);
} catch (...) { return abi_catch(); }

// ------------------------------------------------------------------------------------------------------
// modSwitch building block
// ------------------------------------------------------------------------------------------------------
extern "C" int alch_buf_rescale_drop0(const alch_buf* src, alch_buf* dst, size_t count) try {
    if (!src || !dst) return fail(ALCH_E_INVALID, "null buffer");
    alch_ring* rs = src->ring;
    alch_ring* rd = dst->ring;
    BIND(rs);
    if (rs->L < 2 || rd->L != rs->L - 1 || rd->n != rs->n || rd->word != rs->word)
        return fail(ALCH_E_INVALID, "destination ring must be the source ring minus limb 0");
    for (int j = 1; j < rs->L; ++j)
        if (rs->q[j] != rd->q[j - 1]) return fail(ALCH_E_INVALID, "destination limbs must equal source limbs 1..L-1");
    if (count > src->n_elems || count > dst->n_elems) return fail(ALCH_E_INVALID, "count out of bounds");
    // no overlap check: rd has one limb fewer than rs, so src and dst belong to two rings and to two allocations
    const size_t total = count * (size_t)rd->L * rd->n;
    HIP_TRY(hipStreamSynchronize(rd->stream));
    if (rs->word == 4)
        hipLaunchKernelGGL((k_rescale_drop0<u32>), dim3(ew_grid(total)), dim3(256), 0, rs->stream, rs->d32, (const u32*)src->dptr, (u32*)dst->dptr, count, drop0_inv_mont<u32>(rs, 0));
    else
        hipLaunchKernelGGL((k_rescale_drop0<u64>), dim3(ew_grid(total)), dim3(256), 0, rs->stream, rs->d64, (const u64*)src->dptr, (u64*)dst->dptr, count, drop0_inv_mont<u64>(rs, 0));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(rs->stream));
    return ALCH_OK;
} catch (...) { return abi_catch(); }

extern "C" int alch_buf_rescale_add0(const alch_buf* src, alch_buf* dst, size_t count) try {
    if (!src || !dst) return fail(ALCH_E_INVALID, "null buffer");
    alch_ring* rs = src->ring;
    alch_ring* rd = dst->ring;
    BIND(rd);
    if (rd->L != rs->L + 1 || rd->n != rs->n || rd->word != rs->word)
        return fail(ALCH_E_INVALID, "destination ring must be the source ring plus one limb in front");
    for (int j = 0; j < rs->L; ++j)
        if (rs->q[j] != rd->q[j + 1]) return fail(ALCH_E_INVALID, "destination limbs 1..L must equal the source limbs");
    if (count > src->n_elems || count > dst->n_elems) return fail(ALCH_E_INVALID, "count out of bounds");
    // no overlap check: rd has one limb more than rs, so src and dst belong to two rings and to two allocations
    uint64_t qa[MAXL] = {0};
    for (int j = 1; j < rd->L; ++j) qa[j] = rd->q[0] % rd->q[j];
    const size_t total = count * (size_t)rd->L * rd->n;
    HIP_TRY(hipStreamSynchronize(rs->stream));
    if (rd->word == 4) {
        Scal<u32> sm; scal_to_mont<u32>(rd, qa, 1, sm);
        hipLaunchKernelGGL((k_rescale_add0<u32>), dim3(ew_grid(total)), dim3(256), 0, rd->stream, rd->d32, (const u32*)src->dptr, (u32*)dst->dptr, count, sm);
    } else {
        Scal<u64> sm; scal_to_mont<u64>(rd, qa, 1, sm);
        hipLaunchKernelGGL((k_rescale_add0<u64>), dim3(ew_grid(total)), dim3(256), 0, rd->stream, rd->d64, (const u64*)src->dptr, (u64*)dst->dptr, count, sm);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(rd->stream));
    return ALCH_OK;
} catch (...) { return abi_catch(); }

// ------------------------------------------------------------------------------------------------------
// decrypt and errorRate_ on resident batches (PT2CT.hs:91-99, Eval.hs:150-160): c(s) on the decoding basis, centred lift
// ------------------------------------------------------------------------------------------------------

// Everything alch_buf_lift's kernel needs about (source ring, destination modulus).  rd == null: no residues wanted.
template <typename W>
static LiftPar<W> lift_par(const alch_ring* r, const alch_ring* rd, uint64_t l_scalar) {
    LiftPar<W> P;
    memset(&P, 0, sizeof P);
    const int bits = 8 * (int)sizeof(W);
    P.L = (u32)r->L; P.n = r->n; P.bal = r->balanced ? 1u : 0u;
    P.epw = r->n <= 128 ? 4u : 1u;                                    // up to two coefficients per lane: a wave per element
    for (int j = 0; j < r->L; ++j) {
        P.mod[j] = dev_ring<W>(r).mod[j];
        const u64 qj = r->q[j], r1 = h_powmod(2, (u64)bits, qj);
        for (int i = 0; i < j; ++i) P.inv_m[j][i] = (W)h_mulmod(h_invmod(r->q[i] % qj, qj), r1, qj);
    }
    const u64 p = rd ? rd->q[0] : 2;
    u64 Qp = 1 % p;
    for (int j = 0; j < r->L; ++j) { P.qp[j] = (u32)(r->q[j] % p); Qp = Qp * (r->q[j] % p) % p; }
    P.p = (u32)p; P.Qp = (u32)Qp; P.lmul = (u32)(l_scalar % p); P.pinv = ~(u64)0 / p;
    return P;
}

// Queue the lift of `count` elements at src on r's stream.  dst: 32-bit words of the Z_p ring (or null), maxd: device digits (or null).
template <typename W>
static int launch_lift(alch_ring* r, const alch_ring* rd, const void* src, void* dst, u64* maxd, size_t count, uint64_t l_scalar) {
    if (count == 0 || (!dst && !maxd)) return ALCH_OK;
    const LiftPar<W> P = lift_par<W>(r, dst ? rd : nullptr, l_scalar);
    const size_t per = (size_t)r->L * r->n;
    for (size_t done = 0; done < count;) {                             // grids are 32-bit
        const size_t now = std::min<size_t>(count - done, (size_t)1 << 30);
        hipLaunchKernelGGL((k_lift<W>), dim3((unsigned)((now + P.epw - 1) / P.epw)), dim3(256), 0, r->stream, P,
                           reinterpret_cast<const W*>(src) + done * per, dst ? reinterpret_cast<u32*>(dst) + done * r->n : nullptr,
                           maxd ? maxd + done * (size_t)r->L : nullptr, now);
        done += now;
    }
    HIP_TRY(hipGetLastError());
    return ALCH_OK;
}

// c(s) of `count` ciphertexts at `in` (CRT basis) into `out`, left on the decoding basis: Horner, crtInv, lInv on a general index.
template <typename W>
static int eval_sk_dec(alch_ring* r, const void* in, size_t count, int degree, const void* sk, const uint64_t* s_pre, void* out) {
    Scal<W> s1, s2;
    scal_to_mont<W>(r, s_pre, 1, s1);
    scal_to_mont<W>(r, s_pre, 2, s2);
    const DevRing<W>& R = dev_ring<W>(r);
    constexpr int VL = Vec4<W>::LANES;
    const size_t words = count * elem_words(r);
    W* o = reinterpret_cast<W*>(out);
    const W *i = reinterpret_cast<const W*>(in), *s = reinterpret_cast<const W*>(sk);
    if (r->n % VL == 0) {
        if (degree == 1) hipLaunchKernelGGL((k_ct_eval_sk<W, VL, 1>), dim3(ew_grid(words / VL)), dim3(256), 0, r->stream, R, o, i, s, words, s1, s2);
        else hipLaunchKernelGGL((k_ct_eval_sk<W, VL, 2>), dim3(ew_grid(words / VL)), dim3(256), 0, r->stream, R, o, i, s, words, s1, s2);
    } else {
        if (degree == 1) hipLaunchKernelGGL((k_ct_eval_sk<W, 1, 1>), dim3(ew_grid(words)), dim3(256), 0, r->stream, R, o, i, s, words, s1, s2);
        else hipLaunchKernelGGL((k_ct_eval_sk<W, 1, 2>), dim3(ew_grid(words)), dim3(256), 0, r->stream, R, o, i, s, words, s1, s2);
    }
    HIP_TRY(hipGetLastError());
    if (int rc = do_crt<W>(r, out, 0, count, true)) return rc;
    if (r->gen && r->gh.rad > 1) return do_columns<W>(r, GEN_LINV, out, 0, count, 1);
    return ALCH_OK;
}

// The common body: for chunks of the batch, (crt of a copy of the input with ALCH_POW_IN,) c(s) on the decoding basis into `out` or
// into the ring's scratch, then the lift.  out == null: decrypt_lift; dst == null && maxd == null: error_term.
template <typename W>
static int do_decrypt(alch_ring* r, const void* in, size_t batch, int degree, const void* sk, const uint64_t* s_pre, void* out,
                      const alch_ring* rd, void* dst, uint64_t l_scalar, u64* maxd, bool pow_in) {
    const size_t per = (size_t)degree + 1, eb = elem_bytes(r);
    const size_t per_ct = ((out ? 0 : 1) + (pow_in ? per : 0)) * eb;  // scratch per ciphertext: c(s), the CRT copy of a Pow-basis input
    size_t chunk = batch;
    if (per_ct) {
        chunk = scratch_chunk((size_t)1 << 30, batch, per_ct);
        if (int rc = r->ws_lift.reserve(chunk * per_ct)) return rc;
    }
    Carve cv(r->ws_lift.p, chunk);
    char *ws_cs = cv.take(out ? 0 : eb), *ws_in = cv.take(pow_in ? per * eb : 0);
    if (!cv.matches(per_ct)) return fail(ALCH_E_INTERNAL, "do_decrypt: the scratch carve differs from the bytes reserved per ciphertext");
    for (size_t done = 0; done < batch; done += chunk) {
        const size_t now = std::min(chunk, batch - done);
        const char* src = reinterpret_cast<const char*>(in) + done * per * eb;
        if (pow_in) {
            if (int rc = crt_into<W>(r, ws_in, {src}, now * per, false)) return rc;
            src = ws_in;
        }
        void* cs = out ? reinterpret_cast<char*>(out) + done * eb : ws_cs;
        if (int rc = eval_sk_dec<W>(r, src, now, degree, sk, s_pre, cs)) return rc;
        if (int rc = launch_lift<W>(r, rd, cs, dst ? reinterpret_cast<char*>(dst) + done * (size_t)r->n * 4 : nullptr,
                                    maxd ? maxd + done * (size_t)r->L : nullptr, now, l_scalar)) return rc;
    }
    return ALCH_OK;
}

// Argument checks shared by alch_ct_error_term and alch_ct_decrypt_lift.
static int check_ct_sk(const char* who, const alch_buf* in, size_t batch, int degree, const alch_buf* sk, size_t sk_index, unsigned flags) {
    const std::string w(who);
    if (in->ring != sk->ring) return fail(ALCH_E_INVALID, w + ": the key belongs to another ring than the ciphertexts");
    if (degree != 1 && degree != 2) return fail(ALCH_E_INVALID, w + ": degree must be 1 or 2");
    if (flags & ~(unsigned)ALCH_POW_IN) return fail(ALCH_E_INVALID, w + ": only ALCH_POW_IN is accepted");
    if (batch > in->n_elems / (size_t)(degree + 1)) return fail(ALCH_E_INVALID, w + ": the buffer must hold (degree + 1) * batch ring elements");
    if (sk_index >= sk->n_elems) return fail(ALCH_E_INVALID, w + ": key index out of bounds");
    if (!in->ring->has_crt) return fail(ALCH_E_NO_CRT, w + ": this ring has no CRT basis (created with alch_ring_create_nocrt)");
    return ALCH_OK;
}

// The destination of a lift: one modulus 2 <= p < 2^31 over the source's index.
static int check_lift_dst(const char* who, const alch_ring* r, const alch_buf* dst, size_t dst_first, size_t count) {
    const std::string w(who);
    const alch_ring* rd = dst->ring;
    if (rd->m != r->m || rd->n != r->n) return fail(ALCH_E_INVALID, w + ": the destination ring must have the source's cyclotomic index");
    if (rd->L != 1) return fail(ALCH_E_INVALID, w + ": the destination ring must have exactly one modulus");
    if (rd->zdom || rd->q[0] == 0) return fail(ALCH_E_UNSUPPORTED, w + ": a lift to the integers (q = 0) is not served; lift modulo p");
    if (rd->word != 4 || rd->q[0] >= ((u64)1 << 31)) return fail(ALCH_E_UNSUPPORTED, w + ": the destination modulus must be below 2^31");
    if (rd->device != r->device) return fail(ALCH_E_INVALID, w + ": the rings live on different devices");
    if (!range_ok(dst_first, count, dst->n_elems)) return fail(ALCH_E_INVALID, w + ": destination range out of bounds");
    return ALCH_OK;
}

// Device digits for `count` elements (null when not wanted) / their download into the caller's array.
static int maxd_get(alch_ring* r, const uint64_t* want, size_t count, u64** dev) {
    *dev = nullptr;
    if (!want) return ALCH_OK;
    if (int rc = r->ws_maxd.reserve(count * (size_t)r->L * sizeof(u64))) return rc;
    *dev = reinterpret_cast<u64*>(r->ws_maxd.p);
    return ALCH_OK;
}
static int maxd_fetch(alch_ring* r, uint64_t* host, size_t count) {
    if (!host) return ALCH_OK;
    HIP_TRY(hipMemcpyAsync(host, r->ws_maxd.p, count * (size_t)r->L * sizeof(u64), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return ALCH_OK;
}

extern "C" int alch_ct_error_term(const alch_buf* in, size_t batch, int degree, const alch_buf* sk_crt, size_t sk_index,
                                  const uint64_t* s_pre, alch_buf* out, size_t out_first, unsigned flags) try {
    if (!in || !sk_crt || !out) return fail(ALCH_E_INVALID, "alch_ct_error_term: null buffer");
    alch_ring* r = in->ring;
    BIND(r);
    if (out->ring != r) return fail(ALCH_E_INVALID, "alch_ct_error_term: the output belongs to another ring than the ciphertexts");
    if (int rc = check_ct_sk("alch_ct_error_term", in, batch, degree, sk_crt, sk_index, flags)) return rc;
    if (!range_ok(out_first, batch, out->n_elems)) return fail(ALCH_E_INVALID, "alch_ct_error_term: output range out of bounds");
    if (batch == 0) return ALCH_OK;
    const size_t eb = elem_bytes(r);
    void* o = reinterpret_cast<char*>(out->dptr) + out_first * eb;
    const void* sk = reinterpret_cast<const char*>(sk_crt->dptr) + sk_index * eb;
    if (bytes_overlap(o, batch * eb, in->dptr, batch * (size_t)(degree + 1) * eb) || bytes_overlap(o, batch * eb, sk, eb))
        return fail(ALCH_E_INVALID, "alch_ct_error_term: the output range overlaps an input");
    return ALCH_BY_WORD(r, do_decrypt, r, in->dptr, batch, degree, sk, s_pre, o, nullptr, nullptr, 1, nullptr, (flags & ALCH_POW_IN) != 0);
} catch (...) { return abi_catch(); }

extern "C" int alch_buf_lift(const alch_buf* src, size_t first, size_t count, alch_buf* dst_zp, size_t dst_first, uint64_t l_scalar,
                             uint64_t* max_digits) try {
    if (!src) return fail(ALCH_E_INVALID, "alch_buf_lift: null buffer");
    alch_ring* r = src->ring;
    BIND(r);
    if (!range_ok(first, count, src->n_elems)) return fail(ALCH_E_INVALID, "alch_buf_lift: element range out of bounds");
    if (r->zdom) return fail(ALCH_E_INVALID, "alch_buf_lift: the source is an integer ring already");
    if (!r->has_crt) return fail(ALCH_E_UNSUPPORTED, "alch_buf_lift: the source ring needs prime moduli (a ring created with alch_ring_create)");
    if (dst_zp) if (int rc = check_lift_dst("alch_buf_lift", r, dst_zp, dst_first, count)) return rc;
    if (count == 0 || (!dst_zp && !max_digits)) return ALCH_OK;
    const char* s = reinterpret_cast<const char*>(src->dptr) + first * elem_bytes(r);
    char* d = dst_zp ? reinterpret_cast<char*>(dst_zp->dptr) + dst_first * elem_bytes(dst_zp->ring) : nullptr;
    // the same ring lifting into itself (one limb): in place is fine -- a lane reads its coefficient before it writes it -- shifted is not
    if (d && d != s && bytes_overlap(d, count * elem_bytes(dst_zp->ring), s, count * elem_bytes(r)))
        return fail(ALCH_E_INVALID, "alch_buf_lift: overlapping ranges");
    u64* maxd = nullptr;
    int rc;
    if ((rc = maxd_get(r, max_digits, count, &maxd)) != ALCH_OK) return rc;
    alch_ring* rd = dst_zp ? dst_zp->ring : nullptr;
    if (rd && (rc = ext_order(r, rd, true)) != ALCH_OK) return rc;
    if ((rc = ALCH_BY_WORD(r, launch_lift, r, rd, s, d, maxd, count, l_scalar)) != ALCH_OK) return rc;
    if (rd && (rc = ext_order(r, rd, false)) != ALCH_OK) return rc;
    return maxd_fetch(r, max_digits, count);
} catch (...) { return abi_catch(); }

extern "C" int alch_ct_decrypt_lift(const alch_buf* in, size_t batch, int degree, const alch_buf* sk_crt, size_t sk_index,
                                    const uint64_t* s_pre, alch_buf* dst_zp, size_t dst_first, uint64_t l_scalar, uint64_t* max_digits,
                                    unsigned flags) try {
    if (!in || !sk_crt) return fail(ALCH_E_INVALID, "alch_ct_decrypt_lift: null buffer");
    alch_ring* r = in->ring;
    BIND(r);
    if (int rc = check_ct_sk("alch_ct_decrypt_lift", in, batch, degree, sk_crt, sk_index, flags)) return rc;
    if (dst_zp) if (int rc = check_lift_dst("alch_ct_decrypt_lift", r, dst_zp, dst_first, batch)) return rc;
    if (batch == 0 || (!dst_zp && !max_digits)) return ALCH_OK;
    const void* sk = reinterpret_cast<const char*>(sk_crt->dptr) + sk_index * elem_bytes(r);
    char* d = dst_zp ? reinterpret_cast<char*>(dst_zp->dptr) + dst_first * elem_bytes(dst_zp->ring) : nullptr;
    if (d && (bytes_overlap(d, batch * elem_bytes(dst_zp->ring), in->dptr, batch * (size_t)(degree + 1) * elem_bytes(r)) ||
              bytes_overlap(d, batch * elem_bytes(dst_zp->ring), sk, elem_bytes(r))))
        return fail(ALCH_E_INVALID, "alch_ct_decrypt_lift: the destination range overlaps an input");
    u64* maxd = nullptr;
    int rc;
    if ((rc = maxd_get(r, max_digits, batch, &maxd)) != ALCH_OK) return rc;
    alch_ring* rd = dst_zp ? dst_zp->ring : nullptr;
    if (rd && (rc = ext_order(r, rd, true)) != ALCH_OK) return rc;
    rc = ALCH_BY_WORD(r, do_decrypt, r, in->dptr, batch, degree, sk, s_pre, nullptr, rd, d, l_scalar, maxd, (flags & ALCH_POW_IN) != 0);
    if (rc != ALCH_OK) return rc;
    if (rd && (rc = ext_order(r, rd, false)) != ALCH_OK) return rc;
    return maxd_fetch(r, max_digits, batch);
} catch (...) { return abi_catch(); }

// ------------------------------------------------------------------------------------------------------
// encrypt on resident batches: the counter-based Gaussian on the decoding basis and SymmSHE encrypt's ring arithmetic (kernel_rlwe.hpp)
// ------------------------------------------------------------------------------------------------------
static inline double bits_to_double(uint64_t b) { double d; memcpy(&d, &b, sizeof d); return d; }
static inline uint64_t double_to_bits(double d) { uint64_t b; memcpy(&b, &d, sizeof b); return b; }

extern "C" int alch_gauss_table(uint64_t* cdt, size_t* len) try {
    if (!len) return fail(ALCH_E_INVALID, "alch_gauss_table: null len");
    if (cdt) {
        if (*len < gauss::CDT_LEN) return fail(ALCH_E_INVALID, "alch_gauss_table: the array is shorter than the table (query with cdt = NULL)");
        memcpy(cdt, gauss::CDT, sizeof gauss::CDT);
    }
    *len = gauss::CDT_LEN;
    return ALCH_OK;
} catch (...) { return abi_catch(); }

extern "C" int alch_gauss_plan(uint32_t m, uint64_t svar_bits, uint64_t* scale_bits, uint64_t* chol_bits, size_t* chol_len) try {
    if (m < 1) return fail(ALCH_E_INVALID, "alch_gauss_plan: cyclotomic index must be >= 1");
    if (!gauss::svar_ok(bits_to_double(svar_bits))) return fail(ALCH_E_INVALID, "alch_gauss_plan: svar must be finite and positive");
    if (chol_bits && !chol_len) return fail(ALCH_E_INVALID, "alch_gauss_plan: chol_bits needs chol_len");
    const gauss::Plan P = gauss::make_plan(m, bits_to_double(svar_bits));
    size_t need = 0;
    for (const gauss::Axis& a : P.axes) need += a.Lc.size();
    if (chol_bits) {
        if (*chol_len < need) return fail(ALCH_E_INVALID, "alch_gauss_plan: the array is shorter than the factors (query with chol_bits = NULL)");
        size_t at = 0;
        for (const gauss::Axis& a : P.axes)
            for (double v : a.Lc) chol_bits[at++] = double_to_bits(v);
    }
    if (chol_len) *chol_len = need;
    if (scale_bits) *scale_bits = double_to_bits(P.scale);
    return ALCH_OK;
} catch (...) { return abi_catch(); }

static void launch_gauss_axis(hipStream_t st, const gauss::Axis& a, double* xs, u32 n, u32 cols) {
    GaussChol C;
    memset(&C, 0, sizeof C);
    memcpy(C.l, a.Lc.data(), a.Lc.size() * sizeof(double));
    const dim3 g(ew_grid(cols)), b(256);
    switch (a.p) {
        case 3: hipLaunchKernelGGL((k_gauss_axis<3>), g, b, 0, st, C, xs, n, a.mp, a.stride, cols); break;
        case 5: hipLaunchKernelGGL((k_gauss_axis<5>), g, b, 0, st, C, xs, n, a.mp, a.stride, cols); break;
        case 7: hipLaunchKernelGGL((k_gauss_axis<7>), g, b, 0, st, C, xs, n, a.mp, a.stride, cols); break;
        case 11: hipLaunchKernelGGL((k_gauss_axis<11>), g, b, 0, st, C, xs, n, a.mp, a.stride, cols); break;
        default: hipLaunchKernelGGL((k_gauss_axis<13>), g, b, 0, st, C, xs, n, a.mp, a.stride, cols); break;
    }
}

// Keystream blocks that meet the positions [ctr0, ctr0 + total), total >= 1: the lanes of a keyed Gaussian launch.
static inline size_t keyed_blocks(u64 ctr0, size_t total) { return (size_t)(((ctr0 + total - 1) >> 2) - (ctr0 >> 2) + 1); }

// `count` elements at dst (limb-major words of r), coset: the Z_p words of the first element or null.
template <typename W>
static int do_gauss_dec(alch_ring* r, const gauss::Plan& P, void* dst, size_t count, u32 p, const u32* coset, uint64_t seed, uint64_t elem0) {
    GaussPar G;
    memset(&G, 0, sizeof G);
    for (int j = 0; j < r->L; ++j) G.q[j] = r->q[j];
    G.seed = seed; G.scale = P.scale; G.L = (u32)r->L; G.n = r->n; G.p = p;
    const size_t n = r->n;
    if (P.axes.empty()) {                                              // two-power index: one kernel, no scratch
        while (((u32)1 << G.logn) < r->n) ++G.logn;
        G.ctr0 = elem0 * (u64)n;
        const size_t total = count * n;
        if (r->rng_keyed) {
            const size_t blocks = keyed_blocks(G.ctr0, total);
            hipLaunchKernelGGL((k_gauss_sample_keyed<W, true>), dim3(ew_grid(blocks)), dim3(256), 0, r->stream, G, r->rng_key,
                               (double*)nullptr, reinterpret_cast<W*>(dst), coset, total, blocks);
        } else {
            hipLaunchKernelGGL((k_gauss_sample<W, true>), dim3(ew_grid(total)), dim3(256), 0, r->stream, G, (double*)nullptr,
                               reinterpret_cast<W*>(dst), coset, total);
        }
        HIP_TRY(hipGetLastError());
        return ALCH_OK;
    }
    // scratch of one chunk: at most 1 GiB and fewer than 2^31 coefficients (2^27 doubles)
    const size_t chunk = scratch_chunk((size_t)1 << 30, count, n * sizeof(double));
    if (int rc = r->ws_gauss.reserve(chunk * n * sizeof(double))) return rc;
    double* xs = reinterpret_cast<double*>(r->ws_gauss.p);
    for (size_t done = 0; done < count; done += chunk) {
        const size_t now = std::min(chunk, count - done);
        const u32 total = (u32)(now * n);
        G.ctr0 = (elem0 + (u64)done) * (u64)n;
        if (r->rng_keyed) {
            const size_t blocks = keyed_blocks(G.ctr0, total);
            hipLaunchKernelGGL((k_gauss_sample_keyed<W, false>), dim3(ew_grid(blocks)), dim3(256), 0, r->stream, G, r->rng_key, xs,
                               (W*)nullptr, (const u32*)nullptr, (size_t)total, blocks);
        } else {
            hipLaunchKernelGGL((k_gauss_sample<W, false>), dim3(ew_grid(total)), dim3(256), 0, r->stream, G, xs, (W*)nullptr,
                               (const u32*)nullptr, (size_t)total);
        }
        for (const gauss::Axis& a : P.axes) launch_gauss_axis(r->stream, a, xs, r->n, total / (a.p - 1));
        hipLaunchKernelGGL((k_gauss_round<W>), dim3(ew_grid(total)), dim3(256), 0, r->stream, G, xs,
                           reinterpret_cast<W*>(dst) + done * elem_words(r), coset ? coset + done * n : nullptr, total);
        HIP_TRY(hipGetLastError());
    }
    return ALCH_OK;
}

extern "C" int alch_buf_gauss_dec(alch_buf* dst, size_t first, size_t count, uint64_t svar_bits, const alch_buf* coset_zp,
                                  size_t coset_first, uint64_t seed, uint64_t elem0) try {
    if (!dst) return fail(ALCH_E_INVALID, "alch_buf_gauss_dec: null buffer");
    alch_ring* r = dst->ring;
    BIND(r);
    const double svar = bits_to_double(svar_bits);
    if (!gauss::svar_ok(svar)) return fail(ALCH_E_INVALID, "alch_buf_gauss_dec: svar must be finite and positive");
    if (!range_ok(first, count, dst->n_elems)) return fail(ALCH_E_INVALID, "alch_buf_gauss_dec: element range out of bounds");
    u32 p = 0;
    if (coset_zp) {
        const alch_ring* rc = coset_zp->ring;
        if (rc->m != r->m || rc->n != r->n) return fail(ALCH_E_INVALID, "alch_buf_gauss_dec: the coset ring must have the destination's cyclotomic index");
        if (rc->L != 1 || rc->zdom || rc->word != 4 || rc->q[0] < 2 || rc->q[0] >= ((u64)1 << 31))
            return fail(ALCH_E_INVALID, "alch_buf_gauss_dec: the coset ring must have exactly one modulus 2 <= p < 2^31");
        if (rc->device != r->device) return fail(ALCH_E_INVALID, "alch_buf_gauss_dec: the rings live on different devices");
        if (!range_ok(coset_first, count, coset_zp->n_elems)) return fail(ALCH_E_INVALID, "alch_buf_gauss_dec: coset range out of bounds");
        p = (u32)rc->q[0];
    }
    const gauss::Plan P = gauss::make_plan(r->m, svar);
    if (P.n != r->n) return fail(ALCH_E_INTERNAL, "alch_buf_gauss_dec: ring dimension mismatch");
    for (const gauss::Axis& a : P.axes)
        if (a.p > gauss::MAX_ODD_PRIME) return fail(ALCH_E_UNSUPPORTED, "alch_buf_gauss_dec: odd primes of the index up to 13 are served");
    if (!gauss::bound_ok(P, p)) return fail(ALCH_E_INVALID, "alch_buf_gauss_dec: svar is too large: the rounded coefficients would not stay below 2^62");
    if (r->rng_keyed && !chacha::range_ok((unsigned __int128)elem0 * r->n, (unsigned __int128)count * r->n))
        return fail(ALCH_E_INVALID, "alch_buf_gauss_dec: under a key the positions (elem0 + count) n end at 2^58");
    if (count == 0) return ALCH_OK;
    char* d = reinterpret_cast<char*>(dst->dptr) + first * elem_bytes(r);
    const u32* cs = nullptr;
    if (coset_zp) {
        cs = reinterpret_cast<const u32*>(coset_zp->dptr) + coset_first * (size_t)r->n;
        // the coset in the destination itself (a one-modulus 32-bit ring): in place is fine -- a lane reads its word before it writes it -- shifted is not
        if ((const void*)cs != (const void*)d && bytes_overlap(d, count * elem_bytes(r), cs, count * (size_t)r->n * 4))
            return fail(ALCH_E_INVALID, "alch_buf_gauss_dec: overlapping ranges");
    }
    alch_ring* rc = coset_zp ? coset_zp->ring : nullptr;
    int rcode;
    if (rc && (rcode = ext_order(r, rc, true)) != ALCH_OK) return rcode;
    if ((rcode = ALCH_BY_WORD(r, do_gauss_dec, r, P, d, count, p, cs, seed, elem0)) != ALCH_OK) return rcode;
    if (rc && (rcode = ext_order(r, rc, false)) != ALCH_OK) return rcode;
    return ALCH_OK;
} catch (...) { return abi_catch(); }

template <typename W>
static int do_ct_encrypt(alch_ring* r, void* out, size_t batch, const void* err, const void* sk, uint64_t seed, uint64_t ct0) {
    const DevRing<W>& R = dev_ring<W>(r);
    const size_t words = batch * elem_words(r);
    W* o = reinterpret_cast<W*>(out);
    const W *e = reinterpret_cast<const W*>(err), *s = reinterpret_cast<const W*>(sk);
    if (r->rng_keyed) {                                      // a block per pack of four words when n allows, else a block per word
        if (r->n % 4 == 0) hipLaunchKernelGGL((k_ct_encrypt_keyed<W, 4>), dim3(ew_grid(words / 4)), dim3(256), 0, r->stream, R, r->rng_key, o, e, s, words, seed, ct0);
        else hipLaunchKernelGGL((k_ct_encrypt_keyed<W, 1>), dim3(ew_grid(words)), dim3(256), 0, r->stream, R, r->rng_key, o, e, s, words, seed, ct0);
    } else {
        ALCH_LAUNCH_VW(k_ct_encrypt, r, words, r->stream, R, o, e, s, words, seed, ct0);
    }
    HIP_TRY(hipGetLastError());
    return ALCH_OK;
}

extern "C" int alch_ct_encrypt(alch_buf* out, size_t batch, const alch_buf* err_crt, size_t err_first, const alch_buf* sk_crt,
                               size_t sk_index, uint64_t seed, uint64_t ct0) try {
    if (!out || !err_crt || !sk_crt) return fail(ALCH_E_INVALID, "alch_ct_encrypt: null buffer");
    alch_ring* r = out->ring;
    BIND(r);
    if (err_crt->ring != r || sk_crt->ring != r) return fail(ALCH_E_INVALID, "alch_ct_encrypt: the error terms and the key must belong to the output's ring");
    if (!pairs_ok(batch, out->n_elems)) return fail(ALCH_E_INVALID, "alch_ct_encrypt: the output must hold 2 * batch ring elements");
    if (!range_ok(err_first, batch, err_crt->n_elems)) return fail(ALCH_E_INVALID, "alch_ct_encrypt: error-term range out of bounds");
    if (sk_index >= sk_crt->n_elems) return fail(ALCH_E_INVALID, "alch_ct_encrypt: key index out of bounds");
    if (!r->has_crt) return fail(ALCH_E_NO_CRT, "alch_ct_encrypt: this ring has no CRT basis (created with alch_ring_create_nocrt)");
    if (r->rng_keyed && chacha::odd_pos_end((unsigned __int128)ct0 + batch, (u32)r->L, r->n) > chacha::X_END)
        return fail(ALCH_E_INVALID, "alch_ct_encrypt: under a key the positions 2 (ct0 + batch) L n end at 2^58");
    if (batch == 0) return ALCH_OK;
    const size_t eb = elem_bytes(r);
    const void* e = reinterpret_cast<const char*>(err_crt->dptr) + err_first * eb;
    const void* sk = reinterpret_cast<const char*>(sk_crt->dptr) + sk_index * eb;
    if (bytes_overlap(out->dptr, 2 * batch * eb, e, batch * eb) || bytes_overlap(out->dptr, 2 * batch * eb, sk, eb))
        return fail(ALCH_E_INVALID, "alch_ct_encrypt: the output overlaps an input");
    return ALCH_BY_WORD(r, do_ct_encrypt, r, out->dptr, batch, e, sk, seed, ct0);
} catch (...) { return abi_catch(); }

template <typename W>
static int do_ct_ks_hint(alch_ring* r, const hintgad::Layout& G, void* out, size_t e_first, size_t e_count, const void* v, const void* err,
                         const void* sk, uint64_t seed, uint64_t ct0) {
    const DevRing<W>& R = dev_ring<W>(r);
    const size_t words = e_count * elem_words(r);
    W* o = reinterpret_cast<W*>(out);
    const W *x = reinterpret_cast<const W*>(v), *e = reinterpret_cast<const W*>(err), *s = reinterpret_cast<const W*>(sk);
    if (r->rng_keyed) {
        if (r->n % 4 == 0) hipLaunchKernelGGL((k_ct_ks_hint_keyed<W, 4>), dim3(ew_grid(words / 4)), dim3(256), 0, r->stream, R, r->rng_key, G, o, x, e, s, words, (u64)e_first, seed, ct0);
        else hipLaunchKernelGGL((k_ct_ks_hint_keyed<W, 1>), dim3(ew_grid(words)), dim3(256), 0, r->stream, R, r->rng_key, G, o, x, e, s, words, (u64)e_first, seed, ct0);
    } else {
        ALCH_LAUNCH_VW(k_ct_ks_hint, r, words, r->stream, R, G, o, x, e, s, words, (u64)e_first, seed, ct0);
    }
    HIP_TRY(hipGetLastError());
    return ALCH_OK;
}

// The hint of the values v_crt[v_first ..]: all of it (whole: n_v values, entries 0 .. n_v D) or its entries [e_first, e_first + e_count).
// `name`: the entry point, for the messages.
static int ct_ks_hint(const char* name, bool whole, alch_buf* out, size_t out_first, int gadget, size_t e_first, size_t e_count, size_t n_v,
                      const alch_buf* v_crt, size_t v_first, const alch_buf* err_crt, size_t err_first, const alch_buf* sk_crt,
                      size_t sk_index, uint64_t seed, uint64_t ct0) {
    const std::string who(name);
    if (!out || !v_crt || !err_crt || !sk_crt) return fail(ALCH_E_INVALID, who + ": null buffer");
    alch_ring* r = out->ring;
    BIND(r);
    if (v_crt->ring != r || err_crt->ring != r || sk_crt->ring != r)
        return fail(ALCH_E_INVALID, who + ": the values, the error terms and the key must belong to the output's ring");
    if (gadget_width(gadget) < 0) return fail(ALCH_E_INVALID, who + ": unknown gadget");
    const hintgad::Layout G = hintgad::make_layout_code(r->q, r->L, gadget);
    const size_t D = G.D;
    if (D == 0) return fail(ALCH_E_INVALID, who + ": the gadget has no entries on this ring");
    if (whole) {
        if (n_v > out->n_elems / (2 * D)) return fail(ALCH_E_INVALID, who + ": the output range must hold 2 * n_v * (gadget entries) ring elements");
        e_count = n_v * D;
    } else {                                                 // the values the part's entries belong to
        if (!pairs_ok(e_count, out->n_elems) || e_first > (size_t)-1 - e_count) return fail(ALCH_E_INVALID, who + ": the output range must hold 2 * e_count ring elements");
        n_v = e_count ? (e_first + e_count - 1) / D + 1 : 0;
    }
    if (!pairs_ok(e_count, out->n_elems) || !range_ok(out_first, 2 * e_count, out->n_elems))
        return fail(ALCH_E_INVALID, who + ": the output range must hold 2 ring elements per entry");
    if (!range_ok(v_first, n_v, v_crt->n_elems)) return fail(ALCH_E_INVALID, who + ": value range out of bounds");
    if (!range_ok(err_first, e_count, err_crt->n_elems)) return fail(ALCH_E_INVALID, who + ": error-term range out of bounds");
    if (sk_index >= sk_crt->n_elems) return fail(ALCH_E_INVALID, who + ": key index out of bounds");
    if (!r->has_crt) return fail(ALCH_E_NO_CRT, who + ": this ring has no CRT basis (created with alch_ring_create_nocrt)");
    if (r->rng_keyed && chacha::odd_pos_end((unsigned __int128)ct0 + e_count, (u32)r->L, r->n) > chacha::X_END)
        return fail(ALCH_E_INVALID, who + ": under a key the positions 2 (ct0 + entries) L n end at 2^58");
    if (e_count == 0) return ALCH_OK;
    const size_t eb = elem_bytes(r);
    void* o = reinterpret_cast<char*>(out->dptr) + out_first * eb;
    const void* v = reinterpret_cast<const char*>(v_crt->dptr) + v_first * eb;
    const void* e = reinterpret_cast<const char*>(err_crt->dptr) + err_first * eb;
    const void* sk = reinterpret_cast<const char*>(sk_crt->dptr) + sk_index * eb;
    if (bytes_overlap(o, 2 * e_count * eb, v, n_v * eb) || bytes_overlap(o, 2 * e_count * eb, e, e_count * eb) ||
        bytes_overlap(o, 2 * e_count * eb, sk, eb))
        return fail(ALCH_E_INVALID, who + ": the output overlaps an input");
    return ALCH_BY_WORD(r, do_ct_ks_hint, r, G, o, e_first, e_count, v, e, sk, seed, ct0);
}

extern "C" int alch_ct_ks_hint(alch_buf* out, size_t out_first, int gadget, size_t n_v, const alch_buf* v_crt, size_t v_first,
                               const alch_buf* err_crt, size_t err_first, const alch_buf* sk_crt, size_t sk_index, uint64_t seed,
                               uint64_t ct0) try {
    return ct_ks_hint("alch_ct_ks_hint", true, out, out_first, gadget, 0, 0, n_v, v_crt, v_first, err_crt, err_first, sk_crt, sk_index,
                      seed, ct0);
} catch (...) { return abi_catch(); }

extern "C" int alch_ct_ks_hint_part(alch_buf* out, size_t out_first, int gadget, size_t e_first, size_t e_count, const alch_buf* v_crt,
                                    size_t v_first, const alch_buf* err_crt, size_t err_first, const alch_buf* sk_crt, size_t sk_index,
                                    uint64_t seed, uint64_t ct0) try {
    return ct_ks_hint("alch_ct_ks_hint_part", false, out, out_first, gadget, e_first, e_count, 0, v_crt, v_first, err_crt, err_first, sk_crt,
                      sk_index, seed, ct0);
} catch (...) { return abi_catch(); }

// ------------------------------------------------------------------------------------------------------
// plaintext-side mul_, div2_ and linearCyc_ on resident batches (Eval.hs:65-67, 72-88, 136-148): kernel_plain.hpp
// ------------------------------------------------------------------------------------------------------
// A linear function R_p -> S_p, kept as its values on the (folded) relative basis, lifted, in the CRT basis of the lifting ring.
struct alch_ptlin {
    alch_ring* lift;                           // lifting ring of index s
    u32 m_r, n_r, d_rel;
    u64 p;
    void* ys = nullptr;                        // device: [d_rel][L][n_s], CRT basis, Montgomery form
    int32_t* table = nullptr;                  // device: [d_rel][n_s] source positions in the index-r element, -1 = zero
};

// The exactness bound of include/alchemy_hip.h: terms * phi(m) * 2^(odd primes of m) * floor(p/2)^2.
static int pt_bound(uint32_t m, uint64_t p, uint64_t terms, unsigned __int128* out) {
    if (m < 1 || p < 2 || p >= ((u64)1 << 31)) return fail(ALCH_E_INVALID, "plaintext bound: the modulus must satisfy 2 <= p < 2^31");
    if (terms < 1 || terms > 65536) return fail(ALCH_E_INVALID, "plaintext bound: 1 .. 65536 terms");
    if (!pt_bound_value(m, p, terms, out)) return fail(ALCH_E_INVALID, "plaintext bound: bad argument");      // plain_host.hpp
    return ALCH_OK;
}

extern "C" int alch_pt_bound(uint32_t m, uint64_t p, uint32_t terms, uint64_t* lo, uint64_t* hi) try {
    if (!lo || !hi) return fail(ALCH_E_INVALID, "alch_pt_bound: null argument");
    unsigned __int128 b = 0;
    if (int rc = pt_bound(m, p, terms, &b)) return rc;
    *lo = (uint64_t)b;
    *hi = (uint64_t)(b >> 64);
    return ALCH_OK;
} catch (...) { return abi_catch(); }

// Q / 2 > bound for the lifting ring's Q = prod q_j (Q is odd: Q > 2 bound).
static int pt_check_q(const std::string& who, const alch_ring* lift, uint64_t p, uint64_t terms) {
    unsigned __int128 b = 0;
    if (int rc = pt_bound(lift->m, p, terms, &b)) return rc;
    if (pt_q_exceeds(lift->q, lift->L, b)) return ALCH_OK;
    return fail(ALCH_E_INVALID, who + ": the lifting ring is too small -- Q/2 must exceed terms * phi(m) * 2^(odd primes of m) * (p/2)^2 = 2^" +
                                    std::to_string((int)std::ceil(std::log2((double)b + 1))) + " (terms = " + std::to_string(terms) + ")");
}

// A plaintext buffer's ring: one modulus 2 <= p < 2^31, 32-bit words.
static int pt_check_zp(const std::string& who, const alch_ring* rp) {
    if (rp->L != 1) return fail(ALCH_E_INVALID, who + ": a plaintext ring has exactly one modulus");
    if (rp->zdom || rp->word != 4 || rp->q[0] < 2 || rp->q[0] >= ((u64)1 << 31)) return fail(ALCH_E_INVALID, who + ": the plaintext modulus must satisfy 2 <= p < 2^31");
    return ALCH_OK;
}
static int pt_check_lift(const std::string& who, const alch_ring* lift, const alch_ring* rp) {
    if (rp->m != lift->m || rp->n != lift->n) return fail(ALCH_E_INVALID, who + ": the lifting ring must have the plaintext ring's cyclotomic index");
    if (rp->device != lift->device) return fail(ALCH_E_INVALID, who + ": the rings live on different devices");
    if (!lift->has_crt) return fail(ALCH_E_NO_CRT, who + ": the lifting ring needs a CRT basis (a ring from alch_ring_create)");
    return ALCH_OK;
}

template <typename W>
static int pt_lift_in(alch_ring* lift, void* dst, const void* src, size_t count, u64 p) {
    if (lift->n % 4 == 0)
        hipLaunchKernelGGL((k_pt_lift_in<W, 4>), dim3(ew_grid(count * (size_t)lift->n / 4)), dim3(256), 0, lift->stream, dev_ring<W>(lift), (W*)dst, (const u32*)src, count, (u32)p);
    else
        hipLaunchKernelGGL((k_pt_lift_in<W, 1>), dim3(ew_grid(count * (size_t)lift->n)), dim3(256), 0, lift->stream, dev_ring<W>(lift), (W*)dst, (const u32*)src, count, (u32)p);
    HIP_TRY(hipGetLastError());
    return ALCH_OK;
}

// dst[e] = a[e] * b[e] over the lifting ring, in chunks that keep both lifted operands inside scratch_mib of the ring's scratch.
template <typename W>
static int do_pt_mul(alch_ring* lift, const alch_ring* rp, void* dst, const void* a, const void* b, size_t count) {
    const size_t eb = elem_bytes(lift), zb = (size_t)lift->n * 4;
    const size_t chunk = scratch_chunk(lift->scratch_mib << 20, count, 2 * eb);
    if (int rc = lift->ws_lift.reserve(2 * chunk * eb)) return rc;
    char* A = reinterpret_cast<char*>(lift->ws_lift.p);
    for (size_t done = 0; done < count; done += chunk) {
        const size_t now = std::min(chunk, count - done);
        char* B = A + now * eb;                                       // both operands contiguous: one forward transform launch
        if (int rc = pt_lift_in<W>(lift, A, reinterpret_cast<const char*>(a) + done * zb, now, rp->q[0])) return rc;
        if (int rc = pt_lift_in<W>(lift, B, reinterpret_cast<const char*>(b) + done * zb, now, rp->q[0])) return rc;
        if (int rc = do_crt<W>(lift, A, 0, 2 * now, false)) return rc;
        if (int rc = do_pointwise<W, PW_MUL>(lift, A, A, B, now)) return rc;
        if (int rc = do_crt<W>(lift, A, 0, now, true)) return rc;
        if (int rc = launch_lift<W>(lift, rp, A, reinterpret_cast<char*>(dst) + done * zb, nullptr, now, 1)) return rc;
    }
    return ALCH_OK;
}

extern "C" int alch_pt_mul(alch_ring* lift, alch_buf* dst_zp, const alch_buf* a_zp, const alch_buf* b_zp, size_t count, unsigned flags) try {
    if (!lift || !dst_zp || !a_zp || !b_zp) return fail(ALCH_E_INVALID, "alch_pt_mul: null argument");
    BIND(lift);
    alch_ring* rp = dst_zp->ring;
    if (a_zp->ring != rp || b_zp->ring != rp) return fail(ALCH_E_INVALID, "alch_pt_mul: the three buffers must belong to one plaintext ring");
    if (flags) return fail(ALCH_E_INVALID, "alch_pt_mul: no flag is defined");
    if (int rc = pt_check_zp("alch_pt_mul", rp)) return rc;
    if (int rc = pt_check_lift("alch_pt_mul", lift, rp)) return rc;
    if (!range_ok(0, count, dst_zp->n_elems) || !range_ok(0, count, a_zp->n_elems) || !range_ok(0, count, b_zp->n_elems))
        return fail(ALCH_E_INVALID, "alch_pt_mul: count out of bounds");
    if (int rc = pt_check_q("alch_pt_mul", lift, rp->q[0], 1)) return rc;
    if (count == 0) return ALCH_OK;
    const size_t bytes = count * elem_bytes(rp);
    // dst may be an operand (every chunk is lifted before its results are written); a shifted overlap is refused
    if ((dst_zp->dptr != a_zp->dptr && bytes_overlap(dst_zp->dptr, bytes, a_zp->dptr, bytes)) ||
        (dst_zp->dptr != b_zp->dptr && bytes_overlap(dst_zp->dptr, bytes, b_zp->dptr, bytes)))
        return fail(ALCH_E_INVALID, "alch_pt_mul: the destination overlaps an operand without coinciding with it");
    int rc;
    if ((rc = ext_order(lift, rp, true)) != ALCH_OK) return rc;
    if ((rc = ALCH_BY_WORD(lift, do_pt_mul, lift, rp, dst_zp->dptr, a_zp->dptr, b_zp->dptr, count)) != ALCH_OK) return rc;
    return ext_order(lift, rp, false);
} catch (...) { return abi_catch(); }

extern "C" int alch_pt_linear_free(void* handle) try {
    alch_ptlin* f = reinterpret_cast<alch_ptlin*>(handle);
    if (!f) return ALCH_OK;
    (void)hipSetDevice(f->lift->device);
    (void)hipStreamSynchronize(f->lift->stream);
    if (f->ys) (void)hipFree(f->ys);
    if (f->table) (void)hipFree(f->table);
    delete f;
    return ALCH_OK;
} catch (...) { return abi_catch(); }

extern "C" int alch_pt_linear_create(alch_ring* lift_s, const alch_buf* ys_zp, uint32_t m_r, void** out) try {
    if (!lift_s || !ys_zp || !out) return fail(ALCH_E_INVALID, "alch_pt_linear_create: null argument");
    *out = nullptr;
    BIND(lift_s);
    alch_ring* rp = ys_zp->ring;
    if (m_r < 1) return fail(ALCH_E_INVALID, "alch_pt_linear_create: bad source index");
    if (int rc = pt_check_zp("alch_pt_linear_create", rp)) return rc;
    if (int rc = pt_check_lift("alch_pt_linear_create", lift_s, rp)) return rc;
    u32 e = m_r, t0 = lift_s->m;
    while (t0) { const u32 t = e % t0; e = t0; t0 = t; }
    GenHost ge, gr, gs;
    if (!gen_factor(e, ge) || !gen_factor(m_r, gr) || !gen_factor(lift_s->m, gs)) return fail(ALCH_E_UNSUPPORTED, "alch_pt_linear_create: index not served");
    u32 d_rel = 0, mask = 0;
    std::vector<int32_t> tab;
    if (!gen_tunnel_table(ge, gr, gs, d_rel, tab, mask)) return fail(ALCH_E_INVALID, "alch_pt_linear_create: the indices do not form an extension pair");
    if (ys_zp->n_elems != (size_t)d_rel)
        return fail(ALCH_E_INVALID, "alch_pt_linear_create: ys must hold d_rel = phi(r)/phi(gcd(r, s)) = " + std::to_string(d_rel) + " elements");
    const u64 p = rp->q[0];
    if (int rc = pt_check_q("alch_pt_linear_create", lift_s, p, d_rel)) return rc;
    // x_dec = lInv_R(x_pow), and every E-coefficient goes back through l_E before it is embedded: on the axes of the primes that
    // divide e the two cancel, on the others lInv acts on the RELATIVE index alone (differences y_i - y_(i - m') along that axis).  It
    // is folded into the values once, sum_i y_i (M g)_i = sum_i (M^T y)_i g_i, so that the evaluation gathers Pow coefficients as they
    // are: along each such axis y'_(i0 m' + r) = y_(i0 m' + r) - y_((i0 + 1) m' + r), the last block unchanged.
    const size_t ns = lift_s->n;
    std::vector<int64_t> y((size_t)d_rel * ns);
    int rc = transfer(rp, ys_zp->dptr, 0, d_rel, y.data(), false);
    if (rc != ALCH_OK) return rc;
    BIND(lift_s);
    {
        u32 rel_dim[GEN_MAXFACT];
        for (int l = 0; l < gr.nfact; ++l) {
            int ee = 0;
            for (int le = 0; le < ge.nfact; ++le) if (ge.fact[le].p == gr.fact[l].p) ee = ge.fact[le].e;
            u32 pw = 1;
            for (int k = ee; k < gr.fact[l].e; ++k) pw *= (u32)gr.fact[l].p;
            rel_dim[l] = ee ? pw : gr.fact[l].dim;
        }
        size_t inner = d_rel;                                         // stride (in relative indices) of axis l: product of the later dims
        for (int l = 0; l < gr.nfact; ++l) {
            inner /= rel_dim[l];
            if (mask & (1u << l)) continue;                           // prime divides e: nothing to fold
            const u32 mp = gr.fact[l].mp, dim = rel_dim[l];
            for (size_t i = 0; i < d_rel; ++i) {
                const u32 a = (u32)((i / inner) % dim);
                if (a + mp >= dim) continue;                          // the last block keeps its value
                const int64_t* hi = &y[(i + (size_t)mp * inner) * ns];
                int64_t* lo = &y[i * ns];
                for (size_t k = 0; k < ns; ++k) { const int64_t v = lo[k] - hi[k]; lo[k] = v < 0 ? v + (int64_t)p : v; }
            }
        }
    }
    const int L = lift_s->L;
    std::vector<int64_t> yl((size_t)d_rel * ns * L);
    for (size_t w = 0; w < (size_t)d_rel * ns; ++w) {
        const int64_t v = y[w] % (int64_t)p;
        const int64_t z = v > (int64_t)((p - 1) >> 1) ? v - (int64_t)p : v;
        for (int j = 0; j < L; ++j) {
            const int64_t q = (int64_t)lift_s->q[j];
            int64_t r = z % q;
            yl[w * L + j] = r < 0 ? r + q : r;
        }
    }
    alch_ptlin* f = new alch_ptlin();
    f->lift = lift_s; f->m_r = m_r; f->n_r = gr.n; f->d_rel = d_rel; f->p = p;
    if (hipMalloc(&f->ys, (size_t)d_rel * elem_bytes(lift_s)) != hipSuccess || hipMalloc((void**)&f->table, tab.size() * sizeof(int32_t)) != hipSuccess) {
        alch_pt_linear_free(f);
        return fail(ALCH_E_NOMEM, "hipMalloc(linear function) failed");
    }
    if (hipMemcpy(f->table, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) { alch_pt_linear_free(f); return fail(ALCH_E_HIP, "linear-function table upload failed"); }
    rc = transfer(lift_s, f->ys, 0, d_rel, yl.data(), true);
    if (rc == ALCH_OK) rc = ALCH_BY_WORD(lift_s, do_crt, lift_s, f->ys, 0, d_rel, false);
    if (rc == ALCH_OK) rc = ALCH_BY_WORD(lift_s, tunnel_to_mont, lift_s, f->ys, f->ys, d_rel);
    if (rc != ALCH_OK) { alch_pt_linear_free(f); return rc; }
    if (hipStreamSynchronize(lift_s->stream) != hipSuccess) { alch_pt_linear_free(f); return fail(ALCH_E_HIP, "linear-function setup failed"); }
    *out = f;
    return ALCH_OK;
} catch (...) { return abi_catch(); }

// dst[b] = sum_i y_i * embed(coeffsDec(src[b])_i): gather + lift, forward transforms, inner product, inverse transform, closing lift;
// d_rel + 1 lifting-ring elements of scratch per batch element, chunked under scratch_mib.
template <typename W>
static int do_pt_eval_lin(const alch_ptlin* f, const alch_ring* rd, const void* src, void* dst, size_t count) {
    alch_ring* lift = f->lift;
    const size_t eb = elem_bytes(lift), D = f->d_rel;
    const size_t chunk = scratch_chunk(lift->scratch_mib << 20, count, (D + 1) * eb);
    if (int rc = lift->ws_lift.reserve(chunk * (D + 1) * eb)) return rc;
    char* X = reinterpret_cast<char*>(lift->ws_lift.p);
    for (size_t done = 0; done < count; done += chunk) {
        const size_t now = std::min(chunk, count - done);
        char* O = X + now * D * eb;
        const u32* s = reinterpret_cast<const u32*>(src) + done * (size_t)f->n_r;
        if (lift->n % 4 == 0)
            hipLaunchKernelGGL((k_pt_lift_gather<W, 4>), dim3(ew_grid(now * D * lift->n / 4)), dim3(256), 0, lift->stream, dev_ring<W>(lift), (W*)X, s, f->table, now, (u32)D, f->n_r, (u32)f->p);
        else
            hipLaunchKernelGGL((k_pt_lift_gather<W, 1>), dim3(ew_grid(now * D * lift->n)), dim3(256), 0, lift->stream, dev_ring<W>(lift), (W*)X, s, f->table, now, (u32)D, f->n_r, (u32)f->p);
        HIP_TRY(hipGetLastError());
        if (int rc = do_crt<W>(lift, X, 0, now * D, false)) return rc;
        const size_t words = now * elem_words(lift);
        ALCH_LAUNCH_VW(k_pt_mac, lift, words, lift->stream, dev_ring<W>(lift), (W*)O, (const W*)X, (const W*)f->ys, now, (u32)D);
        HIP_TRY(hipGetLastError());
        if (int rc = do_crt<W>(lift, O, 0, now, true)) return rc;
        if (int rc = launch_lift<W>(lift, rd, O, reinterpret_cast<char*>(dst) + done * (size_t)lift->n * 4, nullptr, now, 1)) return rc;
    }
    return ALCH_OK;
}

extern "C" int alch_pt_eval_lin(const void* handle, const alch_buf* src_zp, alch_buf* dst_zp, size_t count, unsigned flags) try {
    const alch_ptlin* f = reinterpret_cast<const alch_ptlin*>(handle);
    if (!f || !src_zp || !dst_zp) return fail(ALCH_E_INVALID, "alch_pt_eval_lin: null argument");
    alch_ring* lift = f->lift;
    BIND(lift);
    alch_ring *rs = src_zp->ring, *rd = dst_zp->ring;
    if (flags) return fail(ALCH_E_INVALID, "alch_pt_eval_lin: no flag is defined");
    if (int rc = pt_check_zp("alch_pt_eval_lin", rs)) return rc;
    if (int rc = pt_check_zp("alch_pt_eval_lin", rd)) return rc;
    if (rs->q[0] != f->p || rd->q[0] != f->p) return fail(ALCH_E_INVALID, "alch_pt_eval_lin: source and destination carry the modulus of the linear function");
    if (rs->m != f->m_r || rs->n != f->n_r) return fail(ALCH_E_INVALID, "alch_pt_eval_lin: the source ring must have the function's source index");
    if (rs->device != lift->device) return fail(ALCH_E_INVALID, "alch_pt_eval_lin: the rings live on different devices");
    if (int rc = pt_check_lift("alch_pt_eval_lin", lift, rd)) return rc;
    if (!range_ok(0, count, src_zp->n_elems) || !range_ok(0, count, dst_zp->n_elems)) return fail(ALCH_E_INVALID, "alch_pt_eval_lin: count out of bounds");
    if (count == 0) return ALCH_OK;
    if (bytes_overlap(dst_zp->dptr, count * elem_bytes(rd), src_zp->dptr, count * elem_bytes(rs)))
        return fail(ALCH_E_INVALID, "alch_pt_eval_lin: the destination overlaps the source");
    int rc;
    if ((rc = ext_order(lift, rs, true)) != ALCH_OK || (rc = ext_order(lift, rd, true)) != ALCH_OK) return rc;
    if ((rc = ALCH_BY_WORD(lift, do_pt_eval_lin, f, rd, src_zp->dptr, dst_zp->dptr, count)) != ALCH_OK) return rc;
    if ((rc = ext_order(lift, rs, false)) != ALCH_OK) return rc;
    return ext_order(lift, rd, false);
} catch (...) { return abi_catch(); }

extern "C" int alch_pt_rescale(const alch_buf* src_zp, alch_buf* dst_zp, size_t count) try {
    if (!src_zp || !dst_zp) return fail(ALCH_E_INVALID, "alch_pt_rescale: null buffer");
    alch_ring *rs = src_zp->ring, *rd = dst_zp->ring;
    BIND(rd);
    if (int rc = pt_check_zp("alch_pt_rescale", rs)) return rc;
    if (int rc = pt_check_zp("alch_pt_rescale", rd)) return rc;
    if (rs->m != rd->m || rs->n != rd->n) return fail(ALCH_E_INVALID, "alch_pt_rescale: both rings must have one cyclotomic index");
    if (rs->device != rd->device) return fail(ALCH_E_INVALID, "alch_pt_rescale: the rings live on different devices");
    if (rs->q[0] % rd->q[0]) return fail(ALCH_E_INVALID, "alch_pt_rescale: the destination modulus must divide the source modulus");
    if (!range_ok(0, count, src_zp->n_elems) || !range_ok(0, count, dst_zp->n_elems)) return fail(ALCH_E_INVALID, "alch_pt_rescale: count out of bounds");
    if (count == 0) return ALCH_OK;
    const size_t words = count * (size_t)rd->n;
    if (src_zp->dptr != dst_zp->dptr && bytes_overlap(dst_zp->dptr, words * 4, src_zp->dptr, words * 4))
        return fail(ALCH_E_INVALID, "alch_pt_rescale: overlapping ranges");
    const u32 d = (u32)(rs->q[0] / rd->q[0]);
    int rc;
    if ((rc = ext_order(rd, rs, true)) != ALCH_OK) return rc;
    HIP_TRY(hipMemsetAsync(rd->d_flag, 0, sizeof(int), rd->stream));
    if (rd->n % 4 == 0)
        hipLaunchKernelGGL((k_pt_rescale<4>), dim3(ew_grid(words / 4)), dim3(256), 0, rd->stream, (u32*)dst_zp->dptr, (const u32*)src_zp->dptr, words, d, rd->d_flag);
    else
        hipLaunchKernelGGL((k_pt_rescale<1>), dim3(ew_grid(words)), dim3(256), 0, rd->stream, (u32*)dst_zp->dptr, (const u32*)src_zp->dptr, words, d, rd->d_flag);
    HIP_TRY(hipGetLastError());
    if ((rc = ext_order(rd, rs, false)) != ALCH_OK) return rc;
    int flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, rd->d_flag, sizeof(int), hipMemcpyDeviceToHost, rd->stream));
    HIP_TRY(hipStreamSynchronize(rd->stream));
    return flag ? ALCH_NOT_DIVISIBLE : ALCH_OK;
} catch (...) { return abi_catch(); }

template <typename W>
static int do_add_bcast(alch_ring* r, void* dst, const void* src, const void* one, size_t count) {
    const size_t words = count * elem_words(r);
    ALCH_LAUNCH_VW(k_pt_add_bcast, r, words, r->stream, dev_ring<W>(r), (W*)dst, (const W*)src, (const W*)one, words);
    HIP_TRY(hipGetLastError());
    return ALCH_OK;
}

extern "C" int alch_buf_add_bcast(alch_buf* dst, const alch_buf* src, const alch_buf* one, size_t index, size_t count) try {
    if (!dst || !src || !one) return fail(ALCH_E_INVALID, "alch_buf_add_bcast: null buffer");
    alch_ring* r = dst->ring;
    BIND(r);
    if (src->ring != r || one->ring != r) return fail(ALCH_E_INVALID, "alch_buf_add_bcast: buffers belong to different rings");
    if (r->zdom) return fail(ALCH_E_UNSUPPORTED, "alch_buf_add_bcast: not served on the integers");
    if (index >= one->n_elems) return fail(ALCH_E_INVALID, "alch_buf_add_bcast: index out of bounds");
    if (!range_ok(0, count, dst->n_elems) || !range_ok(0, count, src->n_elems)) return fail(ALCH_E_INVALID, "alch_buf_add_bcast: count out of bounds");
    if (count == 0) return ALCH_OK;
    const size_t eb = elem_bytes(r);
    const char* o = reinterpret_cast<const char*>(one->dptr) + index * eb;
    if (bytes_overlap(dst->dptr, count * eb, o, eb) || (dst->dptr != src->dptr && bytes_overlap(dst->dptr, count * eb, src->dptr, count * eb)))
        return fail(ALCH_E_INVALID, "alch_buf_add_bcast: overlapping ranges");
    return ALCH_BY_WORD(r, do_add_bcast, r, dst->dptr, src->dptr, o, count);
} catch (...) { return abi_catch(); }

#include "tensor_ext.inc.hpp"
