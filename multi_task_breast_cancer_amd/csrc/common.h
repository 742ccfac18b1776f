// Shared device/host helpers for the gfx950 kernels.  wave = 64 lanes everywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "../../include/mtbc.h"

#define MTBC_WAVE 64

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define MTBC_CHECK_LAUNCH()                                   \
    do {                                                      \
        hipError_t e__ = hipGetLastError();                   \
        if (e__ != hipSuccess) return MTBC_E_LAUNCH;          \
    } while (0)

// Timing / A-B probes (environment switches, load- / store-skipping bits inside the kernels) exist only in the `make probes`
// build (-DMTBC_PROBES -> libmtbc_hip_probes.so).  The shipped library reads no environment variable: every switch below
// folds to its default at compile time and the probe branches are dead code.
#ifdef MTBC_PROBES
#include <stdlib.h>
static inline int mtbc_probe_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }
static inline bool mtbc_probe_set(const char* name) { return getenv(name) != nullptr; }
#define MTBC_DBG_BIT(p, bit) ((p).dbg & (bit))
#else
#define mtbc_probe_int(name, dflt) (dflt)
#define mtbc_probe_set(name) (false)
#define MTBC_DBG_BIT(p, bit) (0)
#endif

// Per-DEVICE facts (a kernel's opt-in to > 64 KB of dynamic LDS, the CU count, a kernel's resident-block capacity) are remembered per
// device, not per process: one bit / one slot per device ordinal in an atomic owned by the call site.  A process that drives several
// devices sets / queries each of them once; a race repeats an idempotent call.  (Round 3 kept them in `static bool` guards: right for one
// process per GPU, wrong the day one process drives two.)
#include <atomic>
constexpr int MTBC_MAX_DEVICES = 64;
struct DevOnce { std::atomic<unsigned long long> mask{0}; };
static inline int mtbc_current_device() { int dev = 0; return hipGetDevice(&dev) == hipSuccess ? (dev & (MTBC_MAX_DEVICES - 1)) : 0; }
template <typename K> static inline void mtbc_ensure_dyn_lds(DevOnce& once, K kernel, int bytes) {
    const unsigned long long bit = 1ull << mtbc_current_device();
    if (once.mask.load(std::memory_order_relaxed) & bit) return;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    once.mask.fetch_or(bit, std::memory_order_relaxed);
}
#define MTBC_ENSURE_DYN_LDS(kernel, bytes) do { static DevOnce once__; mtbc_ensure_dyn_lds(once__, (kernel), (bytes)); } while (0)
struct DevInts { std::atomic<int> v[MTBC_MAX_DEVICES]; DevInts() { for (auto& x : v) x.store(-1, std::memory_order_relaxed); } };
// value of `query()` on the current device, asked once per device (-1 = not asked yet; query() >= 0)
template <typename F> static inline int mtbc_per_device(DevInts& cache, F&& query) {
    std::atomic<int>& slot = cache.v[mtbc_current_device()];
    int c = slot.load(std::memory_order_relaxed);
    if (c < 0) { c = query(); if (c < 0) c = 0; slot.store(c, std::memory_order_relaxed); }
    return c;
}

static inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// Segment table passed by value to kernels (virtual channel concat).
// Pointers that reach a kernel through LDS (segment tables) lose their address space and would compile to flat_*
// loads / stores (slower, and they tie vmcnt to lgkmcnt); these types put them back into global memory.
#ifdef MTBC_FLAT_AB   // A/B probe only
typedef float gfloat;
typedef char gchar;
#else
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) char gchar;
#endif
typedef __attribute__((address_space(1))) f32x4 gf32x4;

struct SegTable {
    float* ptr[MTBC_MAX_SEGS];
    long long bstride[MTBC_MAX_SEGS];
    int cbegin[MTBC_MAX_SEGS + 1];   // prefix sums of channels; cbegin[n] = total
    int accumulate[MTBC_MAX_SEGS];
    int n;
};

static inline int make_segtable(const mtbc_seg* segs, int n, int expect_channels, SegTable* t) {
    if (n < 1 || n > MTBC_MAX_SEGS) return MTBC_E_BADARG;
    int c = 0;
    for (int i = 0; i < MTBC_MAX_SEGS; ++i) {
        t->ptr[i] = nullptr; t->bstride[i] = 0; t->accumulate[i] = 0; t->cbegin[i] = c;
        if (i < n) {
            if (!segs[i].ptr || segs[i].channels <= 0) return MTBC_E_BADARG;
            t->ptr[i] = segs[i].ptr; t->bstride[i] = segs[i].batch_stride;
            t->accumulate[i] = segs[i].accumulate;
            c += segs[i].channels;
        }
    }
    t->cbegin[MTBC_MAX_SEGS] = c;
    for (int i = n; i <= MTBC_MAX_SEGS; ++i) t->cbegin[i] = c;
    t->n = n;
    return c == expect_channels ? MTBC_OK : MTBC_E_BADSHAPE;
}

// channel c -> its segment (select chain over constant indices: no dynamic kernarg indexing)
struct SegRef { float* ptr; long long bs; int cb; int acc; };
__device__ __forceinline__ SegRef seg_ref(const SegTable& t, int c) {
    SegRef r{t.ptr[0], t.bstride[0], 0, t.accumulate[0]};
#pragma unroll
    for (int i = 1; i < MTBC_MAX_SEGS; ++i) {
        const bool hit = i < t.n && c >= t.cbegin[i];
        r.ptr = hit ? t.ptr[i] : r.ptr;
        r.bs = hit ? t.bstride[i] : r.bs;
        r.cb = hit ? t.cbegin[i] : r.cb;
        r.acc = hit ? t.accumulate[i] : r.acc;
    }
    return r;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The sigmoid of the losses and of every `sigmoid(x) > .5` predicate (head_loss.hip: Dice, dice_counts_kernel; seg_metrics.hip): one
// definition, so a pixel is tumour for all of them or for none.  (__host__ too: mtbc_fill_holes_host compiles the same predicate.)
__host__ __device__ __forceinline__ float sigmoidf_(float v) { return 1.0f / (1.0f + expf(-v)); }

// Source pixel of output pixel (x, y) under RandomHorizontalFlip -> RandomVerticalFlip -> RandomRotation (torchvision: nearest, zero fill,
// centre rotation; the derivation is at the top of augment.hip): false = outside the rotated frame (the output is 0), else (xs, ys) is the pixel to
// read.  ONE definition for augment.hip and batch_loader.hip: the two kernels gather the same pixel, operation for operation.
__device__ __forceinline__ bool flip_rotate_src(int x, int y, int H, int W, float ca, float sa, bool fh, bool fv, int& xs, int& ys) {
    const float xo = (float)x - 0.5f * (float)W + 0.5f, yo = (float)y - 0.5f * (float)H + 0.5f;
    const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;
    const float gx = fmaf(yo, -sa / hw, xo * (ca / hw));
    const float gy = fmaf(yo, ca / hh, xo * (sa / hh));
    const float ix = ((gx + 1.f) * (float)W - 1.f) * 0.5f, iy = ((gy + 1.f) * (float)H - 1.f) * 0.5f;
    const float rx = nearbyintf(ix), ry = nearbyintf(iy);
    const bool inb = rx >= 0.f && rx < (float)W && ry >= 0.f && ry < (float)H;
    xs = inb ? (int)rx : 0; ys = inb ? (int)ry : 0;
    if (fh) xs = W - 1 - xs;
    if (fv) ys = H - 1 - ys;
    return inb;
}

// Block-wide sum; every thread gets the result.  `red` = shared float[17+].  Deterministic.
__device__ __forceinline__ float block_sum(float v, float* red) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = wave_sum(v);
    __syncthreads();                       // protect `red` from a previous use
    if (lane == 0) red[wid] = v;
    __syncthreads();
    float s = 0.f;
    for (int i = 0; i < nw; ++i) s += red[i];
    return s;
}

// Which launches an InstanceNorm + LeakyReLU call makes: the kernel instances (family + template arguments), the block size where the
// dispatcher and not the template fixes it, and the team plan of a cooperative launch.  Every dispatcher of norm.hip / norm_coop.hip
// fills ONE NormChoice first; its launch code then reads the kernels from it, and mtbc_instnorm_kernel_name() -- the same dispatcher
// called with `query` -- prints it: the name cannot drift from the launch (KernelChoice of conv3x3.hip).
enum NormKernel {
    NK_FWD_C8, NK_BWD_C8,                                   // <THREADS, PPT, F16, COOP, ZC8[, DY8]>
    NK_STATS_FIN, NK_APPLY_FWD, NK_BSTATS_FIN, NK_APPLY_BWD,      // the streaming passes: <F16, FIN, ZF16, POOL>, <F16, ZF16>
    NK_R1_FIN, NK_DPARAM,
    NK_FWD_REG, NK_CHUNK_STATS, NK_CHUNK_APPLY, NK_FWD_STREAM, NK_BWD, NK_BWD_REG      // norm.hip: <VPT>, <VEC>, <VPT, BOTH>
};
struct NormLaunch { int k; int t[6]; int threads; int T, rounds; };      // threads > 0: printed as [threads=..]; T > 0: a team launch, [T=.. rounds=..]
struct NormChoice {
    static constexpr int MAX = 4;          // (a call makes at most 3 launches today; one more is a programming error)
    int n; NormLaunch l[MAX];
    void add(int k, int t0 = 0, int t1 = 0, int t2 = 0, int t3 = 0, int t4 = 0, int t5 = 0) { if (n == MAX) abort(); l[n++] = NormLaunch{k, {t0, t1, t2, t3, t4, t5}, 0, 0, 0}; }
    void add(const NormLaunch& k) { if (n == MAX) abort(); l[n++] = k; }
    NormLaunch& last() { return l[n - 1]; }
};
// norm_coop.hip: InstanceNorm straight into the 16-bit channel-blocked layout
// query != NULL: validate, append the launches to *query and return without touching the stream
extern "C" int mtbc_i_instnorm_fwd_c8(const mtbc_instnorm_args* a, hipStream_t st, NormChoice* query);
extern "C" int mtbc_i_instnorm_bwd_c8(const mtbc_instnorm_args* a, float* part, hipStream_t st, NormChoice* query);
extern "C" int mtbc_i_instnorm_bwd_c8_team(const mtbc_instnorm_args* a);
// Which launches a max-pool, 1x1 convolution, GAP, Linear, fused-head, loss or softmax call makes: the dispatchers of pool_up.hip, c8_ops.hip, head_loss.hip
// and the two reducers of reduce.hip take a `query`; with it they validate as the call does, append every launch they would make -- the
// kernel as a profiler spells the instance, then in brackets what the arguments select inside it -- and return without touching the stream
// or the device.  Each decision (the kernel, its template argument, the reducer instance, a block size) is ONE local value that both the
// launch and the query read: mtbc_op_kernel_name() cannot drift from the launch (NormChoice / ConvTChoice below, KernelChoice of conv3x3.hip).
#include <stdarg.h>
#include <stdio.h>
struct OpChoice {
    int n, len; char s[512];
    void add(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
        if (n++ && len < (int)sizeof s - 4) { s[len++] = ' '; s[len++] = '+'; s[len++] = ' '; }
        va_list ap; va_start(ap, fmt);
        const int w = vsnprintf(s + len, sizeof s - len, fmt, ap);
        va_end(ap);
        if (w < 0 || w >= (int)sizeof s - len) abort();          // (a call makes at most five launches with short names; more is a programming error)
        len += w;
    }
};
static inline const char* mtbc_tf(bool b) { return b ? "true" : "false"; }
// c8_ops.hip: max-pool and 1x1 conv on 16-bit channel-blocked tensors
int mtbc_i_maxpool_c8_fwd(const mtbc_maxpool_args* a, hipStream_t st, OpChoice* query);
int mtbc_i_maxpool_c8_bwd(const mtbc_maxpool_args* a, hipStream_t st, OpChoice* query);
int mtbc_i_conv1x1_c8_fwd(const mtbc_conv1x1_args* a, hipStream_t st, OpChoice* query);
size_t mtbc_i_conv1x1_c8_wgrad_workspace(const mtbc_conv1x1_args* a);
int mtbc_i_conv1x1_c8_wgrad(const mtbc_conv1x1_args* a, hipStream_t st, OpChoice* query);
// the entry points of pool_up.hip / head_loss.hip with the query (the extern "C" ones pass NULL)
int mtbc_i_maxpool2_fwd(const mtbc_maxpool_args* a, hipStream_t st, OpChoice* query);
int mtbc_i_maxpool2_bwd(const mtbc_maxpool_args* a, hipStream_t st, OpChoice* query);
int mtbc_i_upsample2_fwd(const mtbc_upsample2_args* a, hipStream_t st, OpChoice* query);
int mtbc_i_upsample2_bwd(const mtbc_upsample2_args* a, hipStream_t st, OpChoice* query);
int mtbc_i_conv1x1_fwd(const mtbc_conv1x1_args* a, hipStream_t st, OpChoice* query);
int mtbc_i_conv1x1_dgrad(const mtbc_conv1x1_args* a, hipStream_t st, OpChoice* query);
int mtbc_i_conv1x1_wgrad(const mtbc_conv1x1_args* a, hipStream_t st, OpChoice* query);
int mtbc_i_head_combine(const mtbc_head_fuse_args* a, hipStream_t st, OpChoice* query);
int mtbc_i_head_expand(const mtbc_head_fuse_args* a, hipStream_t st, OpChoice* query);
int mtbc_i_gap_fwd(const mtbc_gap_args* a, hipStream_t st, OpChoice* query);
int mtbc_i_gap_bwd(const mtbc_gap_args* a, hipStream_t st, OpChoice* query);
int mtbc_i_linear_fwd(const mtbc_linear_args* a, hipStream_t st, OpChoice* query);
int mtbc_i_linear_bwd(const mtbc_linear_args* a, hipStream_t st, OpChoice* query);
int mtbc_i_dice_fwd(const mtbc_dice_args* a, hipStream_t st, OpChoice* query);
int mtbc_i_dice_bwd(const mtbc_dice_args* a, hipStream_t st, OpChoice* query);
int mtbc_i_focal_fwd_bwd(const mtbc_focal_args* a, hipStream_t st, OpChoice* query);
int mtbc_i_loss_mix(const float* seg, const float* cls, float alpha, float* out4, hipStream_t st, OpChoice* query);
int mtbc_i_softmax_rows(const mtbc_softmax_args* a, hipStream_t st, OpChoice* query);
// internal (C++) helpers implemented in reduce.hip; query != NULL: append the launch(es) and return
int mtbc_i_splitk_reduce(const float* partial, float* out, int nsplit, size_t elems, int accumulate, hipStream_t st);
// rows of elems1 + elems2 floats per split: [0, elems1) summed into out, the rest into out2
int mtbc_i_splitk_reduce2(const float* partial, float* out, float* out2, int nsplit, size_t elems1, size_t elems2, int accumulate, hipStream_t st, OpChoice* query = nullptr);
// Which launches a ConvTranspose call makes: the kernel instances (family + template arguments) and the plan facts that select code paths
// inside a kernel without being template arguments.  Every dispatcher of convt2.hip and the ConvT entry points of pool_up.hip fill ONE
// ConvTChoice first; the launch code then reads the kernels from it, and mtbc_convT_kernel_name() -- the same dispatchers called with
// `query` -- prints it: the name cannot drift from the launch (NormChoice above, KernelChoice of conv3x3.hip).
enum ConvTKernel {
    CTK_FWD_LP_C8, CTK_FWD_C8, CTK_FWD_LDS,                  // convt2.hip forward: <MTC, F16>, <KI, F16>, <KI>
    CTK_DGRAD_LDS, CTK_DGRAD2,                               // <LP, D>, <LP, DY16, D>
    CTK_WGRAD16, CTK_WGRAD2, CTK_BWD_FUSED,                  // <LP, CT, D>, <LP, DY16, D>, <LP, CT, NW, ACC>
    CTK_FWD, CTK_DGRAD, CTK_WGRAD,                           // pool_up.hip, the generic GEMM: <KS>
    CTK_SPLITK, CTK_CHANNEL_SUMS                             // reduce.hip follow-ups
};
struct ConvTLaunch { int k; int t[4]; int xcd, splits; };      // xcd: p.xcd_tasks is set; splits > 0: a split-K kernel, printed as [splits=1] / [splits>1]
struct ConvTChoice {
    static constexpr int MAX = 4;          // (a pair makes at most 4 launches: two kernels and two reductions; one more is a programming error)
    int n; ConvTLaunch l[MAX];
    void add(int k, int t0 = 0, int t1 = 0, int t2 = 0, int t3 = 0) { if (n == MAX) abort(); l[n++] = ConvTLaunch{k, {t0, t1, t2, t3}, 0, 0}; }
    void add(const ConvTLaunch& k) { if (n == MAX) abort(); l[n++] = k; }
    ConvTLaunch& last() { return l[n - 1]; }
};
// convt2.hip: ConvTranspose k == s == 2 backward, operands straight from HBM into MFMA fragments
// query != NULL (every launcher below): append the launch to *query and return without touching the stream or the device
bool mtbc_i_convT2_fwd_ok(const mtbc_convT_args* a);
int mtbc_i_convT2_fwd(const mtbc_convT_args* a, hipStream_t st, ConvTChoice* query);
bool mtbc_i_convT2_fwd_c8_ok(const mtbc_convT_args* a);
int mtbc_i_convT2_fwd_c8(const mtbc_convT_args* a, hipStream_t st, ConvTChoice* query);
bool mtbc_i_convT2_fwd_lp_c8_ok(const mtbc_convT_args* a);
int mtbc_i_convT2_fwd_lp_c8(const mtbc_convT_args* a, hipStream_t st, ConvTChoice* query);
bool mtbc_i_convT2_dgrad_ok(const mtbc_convT_args* a);
bool mtbc_i_convT2_wgrad_ok(const mtbc_convT_args* a);
void mtbc_i_convT2_wgrad_plan(const mtbc_convT_args* a, int* steps_per_split, int* nsplit);
int mtbc_i_convT2_dgrad(const mtbc_convT_args* a, int compute, hipStream_t st, ConvTChoice* query);
int mtbc_i_convT2_wgrad(const mtbc_convT_args* a, int compute, float* partial, float* dbias_part, int steps_per_split, int nsplit, hipStream_t st, ConvTChoice* query);
// both gradients of one up-convolution from one read of dy (wg = the OP_CONVT_WGRAD arguments, dg = the OP_CONVT_DGRAD ones)
bool mtbc_i_convT2_bwd_fused_ok(const mtbc_convT_args* wg, const mtbc_convT_args* dg);
int mtbc_i_convT2_bwd_fused(const mtbc_convT_args* wg, const mtbc_convT_args* dg, float* partial, float* dbias_part, int steps_per_split, int nsplit, hipStream_t st, ConvTChoice* query);
// pool_up.hip: a WGRAD op with the DGRAD op of the same up-convolution right behind it; *fused = false: nothing was issued, run them one by one
int mtbc_i_convT_bwd_pair(const mtbc_convT_args* wg, const mtbc_convT_args* dg, void* stream, bool* fused, ConvTChoice* query = nullptr);
int mtbc_i_channel_sums(const float* x, float* planes_ws, float* out, int N, int C, int HW, int accumulate, hipStream_t st, OpChoice* query = nullptr);
