// device_units.hip -- unit tests of the device building blocks, each on the inputs it accepts rather than on the inputs a legal chain
// happens to produce: the wave / block primitives, the generic scan, one radix pass and rs_place, the packed base compares, the K0 kernels.
// A program of its own: it includes the kernel headers of portcullis_amd/csrc, links no library and makes no context.
//   device_units <group>     group = wave | scan | sort | cmp4 | cmp2 | k0
// One line per case, `ok <case>` or `FAIL <case> <what> index <first differing index> got <value> want <value>`, then the number of cases;
// exit status 0 only if every case passed.  A HIP error ends the program at once (status 3).
//   Everything is integer: references are plain host loops in this file and every comparison is exact.  Device functions are called from
// thin wrappers (wk_*, one input per lane, plain stores), kernels are launched as their production callers launch them.  Every output
// buffer lies between two canary regions of one sort tile of 64-bit keys; where a kernel's contract lets it load past the data, that slack
// is allocated and holds a poison pattern.  No case hands a kernel a pointer or a length outside its contract.
#include "../../portcullis_amd/csrc/pjb_kernels.hip.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unistd.h>
#include <vector>

using namespace pjb;

#define CK(x)                                                                                              \
    do {                                                                                                   \
        const hipError_t e_ = (x);                                                                         \
        if (e_ != hipSuccess) {                                                                            \
            fflush(stdout);                                                                                \
            fprintf(stderr, "HIP error at %s:%d: %s (%s)\n", __FILE__, __LINE__, hipGetErrorString(e_), #x); \
            _exit(3);                                                                                      \
        }                                                                                                  \
    } while (0)
static void launched() { // behind every launch: a launch error or a fault ends the program here
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
}

// ---------------------------------------------------------------------------------------------
// cases
// ---------------------------------------------------------------------------------------------
static long g_cases = 0, g_failed = 0;
struct Case {
    std::string name;
    bool bad = false;
    explicit Case(std::string n) : name(std::move(n)) {}
    void miss(const char *what, long idx, unsigned long long got, unsigned long long want) {
        if (bad) return;
        bad = true;
        printf("FAIL %s %s index %ld got %llu want %llu\n", name.c_str(), what, idx, got, want);
    }
    template <typename T>
    void eq(const char *what, const T *got, const T *want, size_t n) {
        for (size_t i = 0; i < n && !bad; i++)
            if (got[i] != want[i]) miss(what, (long)i, (unsigned long long)got[i], (unsigned long long)want[i]);
    }
    template <typename T>
    void eq(const char *what, const std::vector<T> &got, const std::vector<T> &want) {
        if (got.size() != want.size()) miss(what, -1, got.size(), want.size());
        else eq(what, got.data(), want.data(), want.size());
    }
    void flag(const char *what, bool fine) {
        if (!fine) miss(what, -1, 0, 1);
    }
    ~Case() {
        g_cases++;
        if (bad) g_failed++;
        else printf("ok %s\n", name.c_str());
    }
};

// ---------------------------------------------------------------------------------------------
// buffers: [canary | data | slack (poison) | canary]
// ---------------------------------------------------------------------------------------------
static const size_t CANARY = (size_t)RS_TILE * 8; // one sort tile of 64-bit keys
static const uint8_t CANARY_BYTE = 0xC5, POISON_BYTE = 0xA7;
static u32 *g_changed = nullptr; // device: canary / slack bytes found changed
__global__ __launch_bounds__(256) void wk_look(const uint8_t *front, const uint8_t *back, size_t slack, u32 *changed) {
    const size_t n = 2 * CANARY + slack; // the front canary, then the slack and the back canary
    u32 bad = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint8_t got = i < CANARY ? front[i] : back[i - CANARY];
        bad += got != (i < CANARY || i >= CANARY + slack ? CANARY_BYTE : POISON_BYTE);
    }
    if (bad) atomicAdd(changed, bad);
}
struct Guarded {
    uint8_t *raw = nullptr;
    size_t bytes = 0, slack = 0;
    Guarded() {}
    Guarded(size_t b, size_t s = 0) { alloc(b, s); }
    Guarded(const Guarded &) = delete;
    Guarded &operator=(const Guarded &) = delete;
    void alloc(size_t b, size_t s = 0) {
        release();
        bytes = b, slack = s;
        CK(hipMalloc((void **)&raw, 2 * CANARY + bytes + slack + 16));
        CK(hipMemset(raw, CANARY_BYTE, 2 * CANARY + bytes + slack + 16));
        if (slack) CK(hipMemset(raw + CANARY + bytes, POISON_BYTE, slack));
    }
    void release() {
        if (raw) CK(hipFree(raw));
        raw = nullptr;
    }
    ~Guarded() { release(); }
    template <typename T = uint8_t>
    T *p() const { return (T *)(raw + CANARY); }
    void fill(int byte) { // the data
        if (bytes) CK(hipMemset(raw + CANARY, byte, bytes));
    }
    void up(const void *src, size_t n, size_t at = 0) {
        if (n) CK(hipMemcpy(raw + CANARY + at, src, n, hipMemcpyHostToDevice));
    }
    void down(void *dst, size_t n, size_t at = 0) const {
        if (n) CK(hipMemcpy(dst, raw + CANARY + at, n, hipMemcpyDeviceToHost));
    }
    template <typename T>
    std::vector<T> get(size_t n) const {
        std::vector<T> v(n);
        down(v.data(), n * sizeof(T));
        return v;
    }
    // canaries and slack as they were: look() counts the bytes that are not (on the device: a case looks at a dozen buffers), clean()
    // reads the count back and resets it
    void look() const {
        if (!g_changed) {
            CK(hipMalloc((void **)&g_changed, 4));
            CK(hipMemset(g_changed, 0, 4));
        }
        hipLaunchKernelGGL(wk_look, dim3(64), dim3(256), 0, 0, (const uint8_t *)raw, (const uint8_t *)(raw + CANARY + bytes), slack, g_changed);
    }
    static bool clean() {
        u32 changed = 1;
        CK(hipGetLastError());
        CK(hipMemcpy(&changed, g_changed, 4, hipMemcpyDeviceToHost));
        if (changed) CK(hipMemset(g_changed, 0, 4));
        return changed == 0;
    }
    bool intact() const {
        look();
        return clean();
    }
};
template <typename... G>
static bool all_intact(const G &...g) {
    (g.look(), ...);
    return Guarded::clean();
}
template <typename T>
static void upv(Guarded &g, const std::vector<T> &v) {
    if (g.bytes < v.size() * sizeof(T)) g.alloc(v.size() * sizeof(T));
    g.up(v.data(), v.size() * sizeof(T));
}

// splitmix64
struct Rng {
    u64 s;
    explicit Rng(u64 seed) : s(seed) {}
    u64 next() {
        u64 z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    u32 u(u32 n) { return (u32)(next() % n); } // 0 .. n - 1
};
static std::string S(long long v) { return std::to_string(v); }

// =============================================================================================
// group wave
// =============================================================================================
template <typename Op>
__global__ void wk_fold(const u32 *in, u32 *o_fold, u32 *o_total) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    o_fold[i] = wave_fold<Op>(in[i]);
    o_total[i] = wave_total<Op>(in[i]);
}
template <typename T>
__device__ __host__ inline T widen(u32 x) {
    if (sizeof(T) == 8) return (T)((u64)x * 3u + 1u); // (64 of them pass 2^32)
    return (T)x;
}
template <typename T>
__global__ void wk_iscan(const u32 *in, T *out) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    out[i] = wave_iscan<T>(widen<T>(in[i]));
}
__global__ void wk_iscan_dpp(const u32 *in, u32 *out) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    out[i] = wave_iscan_dpp(in[i]);
}
template <typename T, int WHICH>
__global__ void wk_reduce(const u32 *in, T *out) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    const T v = widen<T>(in[i]);
    out[i] = WHICH == 0 ? wave_sum<T>(v) : WHICH == 1 ? wave_max<T>(v) : wave_min<T>(v);
}
template <int NW, typename T, bool LDS_ONLY>
__global__ __launch_bounds__(64 * NW) void wk_escan(const u32 *in, T *ex, T *tot) {
    __shared__ T sm[NW];
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    T t;
    ex[i] = block_escan<NW, T, LDS_ONLY>(widen<T>(in[i]), sm, &t);
    tot[i] = t;
}
template <typename T>
__global__ __launch_bounds__(256) void wk_escan256x2(const u32 *in, T *ex1, T *tot1, T *ex2, T *tot2) { // back to back on one smem, as scan_apply* does
    __shared__ T sm[4];
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    const T v = widen<T>(in[i]);
    T t1, t2;
    const T a = block_escan_256<T>(v, sm, &t1);
    const T b = block_escan_256<T>((T)(v ^ (T)0x5a5a5a5au), sm, &t2);
    ex1[i] = a, tot1[i] = t1, ex2[i] = b, tot2[i] = t2;
}
template <typename OP>
__global__ void wk_seg(const u32 *v, const u32 *key, u32 *out) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    out[i] = seg_reduce_to_head<u32>(v[i], key[i], OP());
}
__global__ __launch_bounds__(256) void wk_hist(const u32 *d, const uint8_t *valid, u32 *out) { // a table per block, as rs_hist keeps it
    __shared__ u32 h[RS_MAX_BINS];
    for (u32 k = threadIdx.x; k < (u32)RS_MAX_BINS; k += blockDim.x) h[k] = 0;
    __syncthreads();
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    wave_hist_add(h, d[i], valid[i] != 0);
    __syncthreads();
    for (u32 k = threadIdx.x; k < (u32)RS_MAX_BINS; k += blockDim.x) out[(size_t)blockIdx.x * RS_MAX_BINS + k] = h[k];
}
template <int BITS>
__global__ void wk_match(const u32 *d, const uint8_t *valid, int bits, u64 *out) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    out[i] = wave_match_digit<BITS>(d[i], valid[i] != 0, bits);
}
__global__ void wk_member(GroupTab T, const int32_t *vpos, int32_t *out) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    const Member M = member_of(T, vpos[i]);
    out[6 * i + 0] = M.idx, out[6 * i + 1] = M.voff, out[6 * i + 2] = M.len, out[6 * i + 3] = M.tid;
    out[6 * i + 4] = (int32_t)(uintptr_t)M.d, out[6 * i + 5] = (int32_t)(uintptr_t)M.codes;
}
__global__ void wk_key(KeyFmt f, const int32_t *s, const int32_t *e, u64 *key, int32_t *s2, int32_t *e2) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    const u64 k = make_key(f, s[i], e[i]);
    key[i] = k;
    int32_t a, b;
    unpack_key(f, k, a, b);
    s2[i] = a, e2[i] = b;
}
__global__ void wk_reach(const u32 *a, u32 *out) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    out[i] = window_reach(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]) ? 1u : 0u;
}

struct HAdd { static u32 op(u32 a, u32 b) { return a + b; } };
struct HMax { static u32 op(u32 a, u32 b) { return a > b ? a : b; } };
struct HMin { static u32 op(u32 a, u32 b) { return a < b ? a : b; } };

static const int WAVE_N = 64 * 64; // 64 waves: "one lane set" has a wave for each lane
struct WaveInput {
    const char *name;
    std::vector<u32> v;
};
static std::vector<WaveInput> wave_inputs() {
    std::vector<WaveInput> in;
    Rng r(11);
    auto add = [&](const char *name, auto f) {
        WaveInput w{name, std::vector<u32>(WAVE_N)};
        for (int i = 0; i < WAVE_N; i++) w.v[i] = f(i);
        in.push_back(std::move(w));
    };
    add("zero", [](int) { return 0u; });
    add("all-ones", [](int) { return 0xffffffffu; });
    add("one-lane", [](int i) { return (i & 63) == (i >> 6) ? 0x80000001u : 0u; }); // wave w: lane w
    add("one-lane-low", [](int i) { return (i & 63) == (i >> 6) ? 0u : 0xfffffff0u; }); // (Min: the one lane below the rest)
    add("ascending", [](int i) { return (u32)i * 3u + 1u; });
    add("random", [&](int) { return (u32)r.next(); });
    add("top-bit", [&](int) { return 0x12345678u | ((u32)(r.next() & 1) << 31); });
    return in;
}

template <typename Op, typename H>
static void wave_fold_case(const std::string &tag, const WaveInput &in, Guarded &din, int bs) {
    Case c("wave " + tag + " block=" + S(bs) + " in=" + in.name);
    Guarded f(WAVE_N * 4), t(WAVE_N * 4);
    hipLaunchKernelGGL(wk_fold<Op>, dim3(WAVE_N / bs), dim3(bs), 0, 0, din.p<u32>(), f.p<u32>(), t.p<u32>());
    launched();
    const auto gf = f.get<u32>(WAVE_N), gt = t.get<u32>(WAVE_N);
    for (int w = 0; w < WAVE_N / 64; w++) {
        u32 want = in.v[w * 64];
        for (int l = 1; l < 64; l++) want = H::op(want, in.v[w * 64 + l]);
        if (gf[w * 64 + 63] != want) c.miss("wave_fold lane 63", w * 64 + 63, gf[w * 64 + 63], want);
        for (int l = 0; l < 64; l++)
            if (gt[w * 64 + l] != want) c.miss("wave_total", w * 64 + l, gt[w * 64 + l], want);
    }
    c.flag("canaries", f.intact() && t.intact());
}
template <typename T>
static void wave_iscan_case(const WaveInput &in, Guarded &din, int bs, bool dpp) {
    Case c(std::string("wave ") + (dpp ? "wave_iscan_dpp" : sizeof(T) == 8 ? "wave_iscan<u64>" : "wave_iscan<u32>") + " block=" + S(bs) + " in=" + in.name);
    Guarded o(WAVE_N * sizeof(T));
    if (dpp) hipLaunchKernelGGL(wk_iscan_dpp, dim3(WAVE_N / bs), dim3(bs), 0, 0, din.p<u32>(), o.p<u32>());
    else hipLaunchKernelGGL(wk_iscan<T>, dim3(WAVE_N / bs), dim3(bs), 0, 0, din.p<u32>(), o.p<T>());
    launched();
    const auto got = o.get<T>(WAVE_N);
    std::vector<T> want(WAVE_N);
    for (int i = 0; i < WAVE_N; i++) want[i] = (T)(((i & 63) ? want[i - 1] : (T)0) + widen<T>(in.v[i]));
    c.eq("inclusive scan", got, want);
    c.flag("canaries", o.intact());
}
template <typename T, int WHICH>
static void wave_reduce_case(const char *tag, const WaveInput &in, Guarded &din, int bs) {
    Case c(std::string("wave ") + tag + " block=" + S(bs) + " in=" + in.name);
    Guarded o(WAVE_N * sizeof(T));
    hipLaunchKernelGGL((wk_reduce<T, WHICH>), dim3(WAVE_N / bs), dim3(bs), 0, 0, din.p<u32>(), o.p<T>());
    launched();
    const auto got = o.get<T>(WAVE_N);
    for (int w = 0; w < WAVE_N / 64; w++) { // (the result is lane 0's)
        T want = widen<T>(in.v[w * 64]);
        for (int l = 1; l < 64; l++) {
            const T x = widen<T>(in.v[w * 64 + l]);
            want = WHICH == 0 ? (T)(want + x) : WHICH == 1 ? (x > want ? x : want) : (x < want ? x : want);
        }
        if (got[w * 64] != want) c.miss("lane 0", w * 64, (unsigned long long)got[w * 64], (unsigned long long)want);
    }
    c.flag("canaries", o.intact());
}
template <int NW, typename T, bool LDS_ONLY>
static void wave_escan_case(const WaveInput &in, Guarded &din) {
    Case c(std::string("wave block_escan<") + S(NW) + (sizeof(T) == 8 ? ",u64," : ",u32,") + (LDS_ONLY ? "true" : "false") + "> in=" + in.name);
    const int bs = 64 * NW;
    Guarded ex(WAVE_N * sizeof(T)), tot(WAVE_N * sizeof(T));
    hipLaunchKernelGGL((wk_escan<NW, T, LDS_ONLY>), dim3(WAVE_N / bs), dim3(bs), 0, 0, din.p<u32>(), ex.p<T>(), tot.p<T>());
    launched();
    const auto ge = ex.get<T>(WAVE_N), gt = tot.get<T>(WAVE_N);
    std::vector<T> we(WAVE_N), wt(WAVE_N);
    for (int b = 0; b < WAVE_N / bs; b++) {
        T run = 0;
        for (int k = 0; k < bs; k++) we[b * bs + k] = run, run = (T)(run + widen<T>(in.v[b * bs + k]));
        for (int k = 0; k < bs; k++) wt[b * bs + k] = run;
    }
    c.eq("exclusive prefix", ge, we);
    c.eq("total", gt, wt);
    c.flag("canaries", ex.intact() && tot.intact());
}
template <typename T>
static void wave_escan256_case(const WaveInput &in, Guarded &din) {
    Case c(std::string("wave block_escan_256<") + (sizeof(T) == 8 ? "u64" : "u32") + "> twice on one smem in=" + in.name);
    Guarded e1(WAVE_N * sizeof(T)), t1(WAVE_N * sizeof(T)), e2(WAVE_N * sizeof(T)), t2(WAVE_N * sizeof(T));
    hipLaunchKernelGGL(wk_escan256x2<T>, dim3(WAVE_N / 256), dim3(256), 0, 0, din.p<u32>(), e1.p<T>(), t1.p<T>(), e2.p<T>(), t2.p<T>());
    launched();
    std::vector<T> we1(WAVE_N), wt1(WAVE_N), we2(WAVE_N), wt2(WAVE_N);
    for (int b = 0; b < WAVE_N / 256; b++) {
        T r1 = 0, r2 = 0;
        for (int k = 0; k < 256; k++) {
            const T v = widen<T>(in.v[b * 256 + k]);
            we1[b * 256 + k] = r1, r1 = (T)(r1 + v);
            we2[b * 256 + k] = r2, r2 = (T)(r2 + (T)(v ^ (T)0x5a5a5a5au));
        }
        for (int k = 0; k < 256; k++) wt1[b * 256 + k] = r1, wt2[b * 256 + k] = r2;
    }
    c.eq("first prefix", e1.get<T>(WAVE_N), we1);
    c.eq("first total", t1.get<T>(WAVE_N), wt1);
    c.eq("second prefix", e2.get<T>(WAVE_N), we2);
    c.eq("second total", t2.get<T>(WAVE_N), wt2);
    c.flag("canaries", e1.intact() && t1.intact() && e2.intact() && t2.intact());
}
template <typename OP, typename H>
static void wave_seg_case(const char *tag, const char *pat, const std::vector<u32> &key, const WaveInput &in, Guarded &din, Guarded &dkey, int bs) {
    Case c(std::string("wave seg_reduce_to_head<") + tag + "> block=" + S(bs) + " segments=" + pat + " in=" + in.name);
    const int n = (int)key.size();
    Guarded o(n * 4);
    hipLaunchKernelGGL(wk_seg<OP>, dim3(n / bs), dim3(bs), 0, 0, din.p<u32>(), dkey.p<u32>(), o.p<u32>());
    launched();
    const auto got = o.get<u32>(n);
    for (int i = 0; i < n; i++) {
        if ((i & 63) && key[i] == key[i - 1]) continue; // not a head
        u32 want = in.v[i];
        for (int j = i + 1; j < (i | 63) + 1 && key[j] == key[i]; j++) want = H::op(want, in.v[j]);
        if (got[i] != want) c.miss("segment head", i, got[i], want);
    }
    c.flag("canaries", o.intact());
}

static void group_wave() {
    const auto inputs = wave_inputs();
    const int shapes[2] = {64, 256};
    for (const auto &in : inputs) {
        Guarded din;
        upv(din, in.v);
        for (int bs : shapes) {
            wave_fold_case<DppAdd, HAdd>("wave_fold/wave_total<DppAdd>", in, din, bs);
            wave_fold_case<DppMax, HMax>("wave_fold/wave_total<DppMax>", in, din, bs);
            wave_fold_case<DppMin, HMin>("wave_fold/wave_total<DppMin>", in, din, bs);
            wave_iscan_case<u32>(in, din, bs, false);
            wave_iscan_case<u32>(in, din, bs, true); // (the same reference: wave_iscan_dpp == wave_iscan<u32>)
            wave_iscan_case<u64>(in, din, bs, false);
            wave_reduce_case<u32, 0>("wave_sum<u32>", in, din, bs);
            wave_reduce_case<u64, 0>("wave_sum<u64>", in, din, bs);
            wave_reduce_case<u32, 1>("wave_max<u32>", in, din, bs);
            wave_reduce_case<int32_t, 1>("wave_max<i32>", in, din, bs);
            wave_reduce_case<u32, 2>("wave_min<u32>", in, din, bs);
            wave_reduce_case<int32_t, 2>("wave_min<i32>", in, din, bs);
        }
        wave_escan_case<1, u32, false>(in, din);
        wave_escan_case<1, u64, false>(in, din);
        wave_escan_case<2, u32, false>(in, din);
        wave_escan_case<2, u64, false>(in, din);
        wave_escan_case<2, u32, true>(in, din);
        wave_escan_case<2, u64, true>(in, din);
        wave_escan_case<4, u32, false>(in, din);
        wave_escan_case<4, u64, false>(in, din);
        wave_escan_case<K1E_T / 64, u32, true>(in, din); // k1_emit's candidate flush
        wave_escan_case<K1E_T / 64, u64, true>(in, din);
        wave_escan256_case<u32>(in, din);
        wave_escan256_case<u64>(in, din);
    }
    { // seg_reduce_to_head: segment patterns, one per wave, every pattern in every wave of the input
        struct Pat {
            const char *name;
            std::vector<int> len; // segment lengths, 64 in all
        };
        std::vector<Pat> pats;
        pats.push_back({"one-of-64", {64}});
        pats.push_back({"64-of-1", std::vector<int>(64, 1)});
        pats.push_back({"1,2,3,...", {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 9}});
        pats.push_back({"31|32", {32, 32}});
        pats.push_back({"62|63", {63, 1}});
        pats.push_back({"31|32,62|63", {7, 25, 31, 1}});
        for (const auto &pt : pats) {
            std::vector<u32> key(WAVE_N);
            for (int w = 0; w < WAVE_N / 64; w++) {
                int l = 0;
                u32 id = 100 + 64 * w; // (a key names one segment: equal keys are contiguous)
                for (int len : pt.len) {
                    for (int k = 0; k < len; k++) key[w * 64 + l++] = id;
                    id++;
                }
            }
            Guarded dkey;
            upv(dkey, key);
            for (const auto &in : inputs) {
                if (!strcmp(in.name, "zero") || !strcmp(in.name, "one-lane-low")) continue;
                Guarded din;
                upv(din, in.v);
                for (int bs : shapes) {
                    wave_seg_case<OpAdd, HAdd>("Add", pt.name, key, in, din, dkey, bs);
                    wave_seg_case<OpMin, HMin>("Min", pt.name, key, in, din, dkey, bs);
                    wave_seg_case<OpMax, HMax>("Max", pt.name, key, in, din, dkey, bs);
                }
            }
        }
    }
    { // wave_hist_add and wave_match_digit: digit patterns over 256-thread blocks
        const int n = 256 * 6;
        Rng r(23);
        struct Dig {
            std::string name;
            std::vector<u32> d;
            int bits; // the digits fit in this width
        };
        std::vector<Dig> digs;
        auto add = [&](const std::string &name, int bits, auto f) {
            Dig g{name, std::vector<u32>(n), bits};
            for (int i = 0; i < n; i++) g.d[i] = f(i) & ((1u << bits) - 1u);
            digs.push_back(std::move(g));
        };
        for (int bits : {1, 4, 9, 10, 11, 12}) {
            const u32 top = 1u << (bits - 1);
            add("one-digit/" + S(bits), bits, [&](int) { return top | 1u; });
            add("two-digits/" + S(bits), bits, [&](int i) { return (i % 5) < 2 ? top : 0u; });
            add("three-interleaved/" + S(bits), bits, [&](int i) { return (u32)(i % 3) * (top | 1u); });
            add("64-distinct/" + S(bits), bits, [&](int i) { return (u32)(i & 63) * 37u + (u32)(i >> 6); }); // (distinct from 9 bits on)
            add("top-bit-only/" + S(bits), bits, [&](int) { return ((top - 1u) & 0x2a5u) | (r.next() & 1 ? top : 0u); });
            add("random/" + S(bits), bits, [&](int) { return (u32)r.next(); });
        }
        std::vector<uint8_t> all(n, 1), half(n);
        for (int i = 0; i < n; i++) half[i] = (uint8_t)(r.next() & 1);
        Guarded dall, dhalf;
        upv(dall, all), upv(dhalf, half);
        for (const auto &g : digs) {
            Guarded dd;
            upv(dd, g.d);
            for (int hv = 0; hv < 2; hv++) {
                const std::vector<uint8_t> &valid = hv ? half : all;
                const Guarded &dv = hv ? dhalf : dall;
                const std::string vn = hv ? " valid=random-half" : " valid=all";
                {
                    Case c("wave wave_hist_add digits=" + g.name + vn);
                    Guarded o((size_t)(n / 256) * RS_MAX_BINS * 4);
                    hipLaunchKernelGGL(wk_hist, dim3(n / 256), dim3(256), 0, 0, dd.p<u32>(), dv.p<uint8_t>(), o.p<u32>());
                    launched();
                    std::vector<u32> want((size_t)(n / 256) * RS_MAX_BINS, 0);
                    for (int i = 0; i < n; i++)
                        if (valid[i]) want[(size_t)(i / 256) * RS_MAX_BINS + g.d[i]]++;
                    c.eq("table", o.get<u32>(want.size()), want);
                    c.flag("canaries", o.intact());
                }
                for (int inst : {0, 9, 10, 11}) {
                    if (inst && inst != g.bits) continue;
                    Case c("wave wave_match_digit<" + S(inst) + "> bits=" + S(g.bits) + " digits=" + g.name + vn);
                    Guarded o((size_t)n * 8);
                    if (inst == 0) hipLaunchKernelGGL(wk_match<0>, dim3(n / 256), dim3(256), 0, 0, dd.p<u32>(), dv.p<uint8_t>(), g.bits, o.p<u64>());
                    if (inst == 9) hipLaunchKernelGGL(wk_match<9>, dim3(n / 256), dim3(256), 0, 0, dd.p<u32>(), dv.p<uint8_t>(), g.bits, o.p<u64>());
                    if (inst == 10) hipLaunchKernelGGL(wk_match<10>, dim3(n / 256), dim3(256), 0, 0, dd.p<u32>(), dv.p<uint8_t>(), g.bits, o.p<u64>());
                    if (inst == 11) hipLaunchKernelGGL(wk_match<11>, dim3(n / 256), dim3(256), 0, 0, dd.p<u32>(), dv.p<uint8_t>(), g.bits, o.p<u64>());
                    launched();
                    const auto got = o.get<u64>(n);
                    for (int i = 0; i < n; i++) {
                        if (!valid[i]) continue; // (a lane that is not valid has no peers to speak of)
                        u64 want = 0;
                        for (int l = 0; l < 64; l++) {
                            const int j = (i & ~63) + l;
                            if (valid[j] && g.d[j] == g.d[i]) want |= 1ull << l;
                        }
                        if (got[i] != want) c.miss("peers", i, got[i], want);
                    }
                    c.flag("canaries", o.intact());
                }
            }
        }
    }
    for (int n : {1, 2, 31, 32}) { // member_of
        Case c("wave member_of n=" + S(n));
        GroupTab T;
        memset(&T, 0, sizeof(T));
        T.n = n;
        int32_t at = 0;
        for (int m = 0; m < n; m++) {
            T.voff[m] = at, T.len[m] = 1000 + 77 * m, T.tid[m] = 100 + m;
            T.d[m] = (const uint8_t *)(uintptr_t)(0x1000u * (m + 1)), T.codes[m] = (const u32 *)(uintptr_t)(0x2000u * (m + 1)); // (never followed)
            at = (at + T.len[m] + GROUP_GAP + 63) & ~63;
        }
        std::vector<int32_t> q;
        for (int m = 0; m < n; m++) q.push_back(T.voff[m] - 1), q.push_back(T.voff[m]), q.push_back(T.voff[m] + T.len[m] - 1);
        const size_t real = q.size();
        while (q.size() % 64) q.push_back(q.back());
        Guarded dq, o(q.size() * 24);
        upv(dq, q);
        hipLaunchKernelGGL(wk_member, dim3(q.size() / 64), dim3(64), 0, 0, T, dq.p<int32_t>(), o.p<int32_t>());
        launched();
        const auto got = o.get<int32_t>(q.size() * 6);
        for (size_t i = 0; i < real; i++) {
            int m = 0;
            for (int k = 1; k < n; k++)
                if (T.voff[k] <= q[i]) m = k;
            const int32_t want[6] = {m, T.voff[m], T.len[m], T.tid[m], (int32_t)(0x1000u * (m + 1)), (int32_t)(0x2000u * (m + 1))};
            for (int k = 0; k < 6; k++)
                if (got[6 * i + k] != want[k]) c.miss("member field", (long)(6 * i + k), (u32)got[6 * i + k], (u32)want[k]);
        }
        c.flag("canaries", o.intact());
    }
    for (int lbits = 0; lbits <= 31; lbits++) { // make_key / unpack_key (lbits 0: the raw format)
        Case c(lbits ? "wave make_key/unpack_key packed lbits=" + S(lbits) : std::string("wave make_key/unpack_key raw"));
        KeyFmt f;
        f.raw = lbits == 0, f.lbits = lbits, f.total_bits = lbits ? 31 + lbits : 64;
        std::vector<int32_t> s, e;
        Rng r(100 + lbits);
        const int32_t top = 0x7fffffff;
        if (lbits == 0) {
            for (int32_t a : {0, 1, top, 5}) for (int32_t b : {0, 1, top, 4}) s.push_back(a), e.push_back(b);
            for (int k = 0; k < 40; k++) s.push_back((int32_t)(r.next() & 0x7fffffff)), e.push_back((int32_t)(r.next() & 0x7fffffff));
        } else {
            const int64_t lmax = ((int64_t)1 << lbits) - 1; // the longest intron the format holds
            for (int64_t len : {(int64_t)1, (int64_t)2, lmax / 2 + 1, lmax}) {
                if (len < 1 || len > lmax) continue;
                const int32_t smax = (int32_t)(top - (len - 1)); // the largest start that leaves room for it
                for (int32_t st : {0, 1, smax, smax / 2, (int32_t)(r.next() % ((u64)smax + 1))}) s.push_back(st), e.push_back((int32_t)(st + len - 1));
            }
        }
        const size_t real = s.size();
        while (s.size() % 64) s.push_back(s.back()), e.push_back(e.back());
        Guarded ds, de, dk(s.size() * 8), s2(s.size() * 4), e2(s.size() * 4);
        upv(ds, s), upv(de, e);
        hipLaunchKernelGGL(wk_key, dim3(s.size() / 64), dim3(64), 0, 0, f, ds.p<int32_t>(), de.p<int32_t>(), dk.p<u64>(), s2.p<int32_t>(), e2.p<int32_t>());
        launched();
        const auto gk = dk.get<u64>(s.size());
        const auto gs = s2.get<int32_t>(s.size()), ge = e2.get<int32_t>(s.size());
        for (size_t i = 0; i < real; i++) {
            const u64 want = lbits == 0 ? ((u64)(u32)s[i] << 32) | (u32)e[i] : ((u64)(u32)s[i] << lbits) | (u64)(u32)(e[i] - s[i] + 1);
            if (gk[i] != want) c.miss("key", (long)i, gk[i], want);
            if (gs[i] != s[i]) c.miss("start", (long)i, (u32)gs[i], (u32)s[i]);
            if (ge[i] != e[i]) c.miss("end", (long)i, (u32)ge[i], (u32)e[i]);
        }
        c.flag("canaries", dk.intact() && s2.intact() && e2.intact());
    }
    { // window_reach at the saturation edges
        Case c("wave window_reach");
        const u32 M = 0xffffffffu;
        std::vector<u32> a;
        const u32 blks[] = {0, 1, 100, 0x7fffffffu, 0x80000000u, M - 1, M};
        const u32 nls[] = {0, 1, 99, 0x7fffffffu, 0x80000000u, M - 1, M};
        const u32 Bs[] = {0, 1, 100, 199, 200, 0x7fffffffu, M - 2, M - 1, M};
        for (u32 blk : blks) for (u32 p : nls) for (u32 q : nls) for (u32 B : Bs) a.insert(a.end(), {blk, p, q, B});
        for (u32 B : Bs) // blk + nl = 2^32 - 1 and 2^32 exactly
            for (u32 blk : {1u, 0x80000000u, M - 1}) {
                a.insert(a.end(), {blk, M - blk, M, B}), a.insert(a.end(), {blk, M - blk + 1, M, B});
                a.insert(a.end(), {blk, M, M - blk - 1, B}), a.insert(a.end(), {blk, M, M - blk, B});
            }
        const size_t real = a.size() / 4;
        while ((a.size() / 4) % 64) a.insert(a.end(), {0, 0, 0, 0});
        Guarded da, o(a.size());
        upv(da, a);
        hipLaunchKernelGGL(wk_reach, dim3(a.size() / 4 / 64), dim3(64), 0, 0, da.p<u32>(), o.p<u32>());
        launched();
        const auto got = o.get<u32>(a.size() / 4);
        for (size_t i = 0; i < real; i++) {
            const u64 blk = a[4 * i], p = a[4 * i + 1], q = a[4 * i + 2], B = a[4 * i + 3];
            // (the rule in 64 bits; an all-ones B lists every read, which is what a saturated sum must come to)
            const u32 want = (B == M || blk + p <= B || blk + q + 1 <= B) ? 1u : 0u;
            if (got[i] != want) c.miss("reach", (long)i, got[i], want);
        }
        c.flag("canaries", o.intact());
    }
}

#include "units_scan.hip.h"
#include "units_sort.hip.h"
#include "units_cmp.hip.h"
#include "units_k0.hip.h"

int main(int argc, char **argv) {
    struct Group {
        const char *name;
        void (*run)();
    };
    const Group groups[] = {{"wave", group_wave}, {"scan", group_scan}, {"sort", group_sort}, {"cmp4", group_cmp4}, {"cmp2", group_cmp2}, {"k0", group_k0}};
    const Group *g = nullptr;
    for (const Group &k : groups)
        if (argc == 2 && !strcmp(argv[1], k.name)) g = &k;
    if (!g) {
        fprintf(stderr, "usage: %s wave|scan|sort|cmp4|cmp2|k0\n", argv[0]);
        return 2;
    }
    setvbuf(stdout, nullptr, _IOLBF, 0);
    CK(hipSetDevice(0));
    g->run();
    CK(hipDeviceSynchronize());
    printf("%s: %ld cases, %ld failed\n", g->name, g_cases, g_failed);
    return g_failed ? 1 : 0;
}
