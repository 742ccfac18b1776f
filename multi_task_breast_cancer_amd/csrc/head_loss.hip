// Pooled classification head (GAP + Linear), fused Dice / Focal losses, loss mix + NaN flag,
// fused Adam / SGD / AdamW (one kernel) and the train-loop Dice counters.  All HBM-/latency-bound; reductions use wavefront
// shuffles (64 lanes) then LDS across waves -- deterministic, no float atomics.
#include "common.h"
#include <atomic>
#include <cstring>

namespace {

// ------------------------------------------------------------------ GAP (one wave per plane)
__global__ void gap_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int planes, int HW) {
    const int plane = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (plane >= planes) return;
    const float* src = x + (size_t)plane * HW;
    float s = 0.f;
    for (int i = lane; i < HW; i += 64) s += src[i];
    s = wave_sum(s);
    if (lane == 0) y[plane] = s / (float)HW;
}
__global__ void gap_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, size_t total, int HW) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) dx[i] = dy[i / HW] / (float)HW;
}

// ------------------------------------------------------------------ Linear (one wave per output)
__global__ void linear_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                  float* __restrict__ y, int N, int In, int Out, int relu) {
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (o >= N * Out) return;
    const int n = o / Out, oc = o % Out;
    float s = 0.f;
    for (int i = lane; i < In; i += 64) s = fmaf(x[(size_t)n * In + i], w[(size_t)oc * In + i], s);
    s = wave_sum(s);
    if (lane == 0) {
        s += b ? b[oc] : 0.f;
        y[o] = (relu && s < 0.f) ? 0.f : s;
    }
}
// g = dy * (relu ? y > 0 : 1)
__global__ void linear_mask_kernel(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ g, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) g[i] = y[i] > 0.f ? dy[i] : 0.f;
}
__global__ void linear_dx_kernel(const float* __restrict__ g, const float* __restrict__ w, float* __restrict__ dx, int N,
                                 int In, int Out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * In) return;
    const int n = idx / In, i = idx % In;
    float s = 0.f;
    int o = 0;
    for (; o + 8 <= Out; o += 8) {           // sixteen loads in flight, the fma chain in the plain loop's order (one round trip per o otherwise)
        float gv[8], wv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { gv[u] = g[(size_t)n * Out + o + u]; wv[u] = w[(size_t)(o + u) * In + i]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) s = fmaf(gv[u], wv[u], s);
    }
    for (; o < Out; ++o) s = fmaf(g[(size_t)n * Out + o], w[(size_t)o * In + i], s);
    dx[idx] = s;
}
__global__ void linear_dw_kernel(const float* __restrict__ g, const float* __restrict__ x, float* __restrict__ dw,
                                 float* __restrict__ db, int N, int In, int Out, int accumulate) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < Out * In) {
        const int o = idx / In, i = idx % In;
        float s = 0.f;
        int n = 0;
        for (; n + 8 <= N; n += 8) {
            float gv[8], xv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { gv[u] = g[(size_t)(n + u) * Out + o]; xv[u] = x[(size_t)(n + u) * In + i]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) s = fmaf(gv[u], xv[u], s);
        }
        for (; n < N; ++n) s = fmaf(g[(size_t)n * Out + o], x[(size_t)n * In + i], s);
        dw[idx] = accumulate ? dw[idx] + s : s;
    }
    if (db && idx < Out) {
        float s = 0.f;
        for (int n = 0; n < N; ++n) s += g[(size_t)n * Out + idx];
        db[idx] = accumulate ? db[idx] + s : s;
    }
}

// ------------------------------------------------------------------ Linear on a wide input: batch-shared kernels (mtbc.h, MTBC_LINEAR_WIDE_MIN_IN)
// The per-sample kernels above stream the whole weight matrix once per sample (50 MB at In = 49152, Out = 256).  Here a wave owns a slab of W
// and ALL samples, LW_NB at a time in registers: W comes from memory once per launch (further passes of a batch larger than LW_NB find their
// slab in the cache).  Both split their reduction dimension over blockIdx.y and leave fp32 partials that a second launch sums in split
// order: the same bits every run, no atomics.  In % 4 == 0 and 16-byte aligned rows: every W access is a float4.
constexpr int LW_NB = 8;      // samples per pass
constexpr int LW_OT = 4;      // forward: output rows per wave (each x float4 is used LW_OT times)

// forward: block = one wave = rows [4 bx, 4 bx + 4) of W x columns [by * kchunk, + kchunk) x all samples -> part[by][n][o]
__global__ __launch_bounds__(64) void linear_wide_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ part,
                                                             int N, int In, int Out, int kchunk) {
    const int lane = threadIdx.x, o0 = blockIdx.x * LW_OT, s = blockIdx.y;
    const int k0 = s * kchunk, k1 = min(In, k0 + kchunk);
    const float4* wr[LW_OT];
#pragma unroll
    for (int t = 0; t < LW_OT; ++t) wr[t] = reinterpret_cast<const float4*>(w + (size_t)min(o0 + t, Out - 1) * In);      // a row past Out re-reads the last one; never stored
    for (int n0 = 0; n0 < N; n0 += LW_NB) {
        float acc[LW_OT][LW_NB];
#pragma unroll
        for (int t = 0; t < LW_OT; ++t)
#pragma unroll
            for (int j = 0; j < LW_NB; ++j) acc[t][j] = 0.f;
        for (int k = k0 + 4 * lane; k < k1; k += 256) {
            float4 wv[LW_OT];
#pragma unroll
            for (int t = 0; t < LW_OT; ++t) wv[t] = wr[t][k >> 2];
#pragma unroll
            for (int j = 0; j < LW_NB; ++j) {
                if (n0 + j < N) {        // uniform over the wave
                    const float4 xv = *reinterpret_cast<const float4*>(x + (size_t)(n0 + j) * In + k);
#pragma unroll
                    for (int t = 0; t < LW_OT; ++t)
                        acc[t][j] = fmaf(xv.w, wv[t].w, fmaf(xv.z, wv[t].z, fmaf(xv.y, wv[t].y, fmaf(xv.x, wv[t].x, acc[t][j]))));
                }
            }
        }
#pragma unroll
        for (int t = 0; t < LW_OT; ++t)
#pragma unroll
            for (int j = 0; j < LW_NB; ++j) {
                const float v = wave_sum(acc[t][j]);
                if (lane == 0 && o0 + t < Out && n0 + j < N) part[((size_t)s * N + n0 + j) * Out + o0 + t] = v;
            }
    }
}
// y[n][o] = relu?(bias[o] + sum_s part[s][n][o]), s ascending
__global__ void linear_wide_reduce_kernel(const float* __restrict__ part, const float* __restrict__ b, float* __restrict__ y, int S, int NO,
                                          int Out, int relu) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= NO) return;
    float s = 0.f;
    for (int k = 0; k < S; ++k) s += part[(size_t)k * NO + i];
    s += b ? b[i % Out] : 0.f;
    y[i] = (relu && s < 0.f) ? 0.f : s;
}
// dx: thread = one float4 column of W x outputs [by * ochunk, + ochunk) x all samples -> dst[by][n][i] (dst = dx itself when there is one split)
__global__ __launch_bounds__(64) void linear_wide_dx_kernel(const float* __restrict__ g, const float* __restrict__ w, float* __restrict__ dst,
                                                            int N, int In, int Out, int ochunk) {
    const int In4 = In >> 2, i4 = blockIdx.x * 64 + threadIdx.x;
    if (i4 >= In4) return;
    const int s = blockIdx.y, o0 = s * ochunk, o1 = min(Out, o0 + ochunk);
    const float4* w4 = reinterpret_cast<const float4*>(w) + i4;
    for (int n0 = 0; n0 < N; n0 += LW_NB) {
        float4 acc[LW_NB];
#pragma unroll
        for (int j = 0; j < LW_NB; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        int o = o0;
        for (; o + 4 <= o1; o += 4) {          // four rows of W in flight
            float4 wv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) wv[u] = w4[(size_t)(o + u) * In4];
#pragma unroll
            for (int j = 0; j < LW_NB; ++j) {
                if (n0 + j < N) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const float gv = g[(size_t)(n0 + j) * Out + o + u];
                        acc[j].x = fmaf(gv, wv[u].x, acc[j].x); acc[j].y = fmaf(gv, wv[u].y, acc[j].y);
                        acc[j].z = fmaf(gv, wv[u].z, acc[j].z); acc[j].w = fmaf(gv, wv[u].w, acc[j].w);
                    }
                }
            }
        }
        for (; o < o1; ++o) {
            const float4 wv = w4[(size_t)o * In4];
#pragma unroll
            for (int j = 0; j < LW_NB; ++j) {
                if (n0 + j < N) {
                    const float gv = g[(size_t)(n0 + j) * Out + o];
                    acc[j].x = fmaf(gv, wv.x, acc[j].x); acc[j].y = fmaf(gv, wv.y, acc[j].y);
                    acc[j].z = fmaf(gv, wv.z, acc[j].z); acc[j].w = fmaf(gv, wv.w, acc[j].w);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < LW_NB; ++j)
            if (n0 + j < N) reinterpret_cast<float4*>(dst + ((size_t)s * N + n0 + j) * In)[i4] = acc[j];
    }
}
// dx[e] = sum_s part[s][e], s ascending; e over the N * In / 4 float4 of dx
__global__ void linear_wide_dx_reduce_kernel(const float4* __restrict__ part, float4* __restrict__ dx, int S, size_t total4) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total4) return;
    float4 s = part[i];
    for (int k = 1; k < S; ++k) { const float4 v = part[(size_t)k * total4 + i]; s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }
    dx[i] = s;
}

// ------------------------------------------------------------------ segmentation criteria (Dice, BCE, Dice+Focal, Jaccard)
// One pair of launches for every criterion; the criterion is a compile-time KIND (mtbc_dice_args.kind):
//   0 DICE       monai DiceLoss(sigmoid, squared_pred, smooth nr/dr): stats {I = sum p t, sum p^2, sum t^2}, mean over planes
//   1 BCE        torch.nn.BCEWithLogitsLoss(): stats {sum bce}, bce = (1 - t) x + softplus(-x), mean over all elements
//   2 FocalDICE  monai 1.3.0 DiceFocalLoss(sigmoid, squared_pred, smooth nr/dr, gamma, no alpha, lambda 1/1): kind 0's term plus the mean over all
//                elements of m * bce, m = exp(gamma * logsigmoid(-x s)), s = 2 t - 1: stats {I, sum p^2, sum t^2, sum focal}
//   3 Jaccard    monai DiceLoss(sigmoid, jaccard=True, reduction="sum"): stats {I, P = sum p, T = sum t}, f = 1 - (2 I + nr) / (2 (P + T - I) + dr),
//                SUMMED over planes (no 1 / planes in the loss or in the gradient)
// The MONAI formulas are restated from knowledge of MONAI 1.3.0 (no MONAI checkout here): re-verify against one, as DESIGN.md says for DiceLoss.
// Kind 0 is the Dice kernel as it was, operation for operation; the others keep its structure (16-byte loads, four rounds in flight, a scalar
// fallback, one block per (plane, head), block_sum reductions, an elementwise backward that reads the plane's statistics).
struct DiceP {
    int n_heads, planes, HW;
    float nr, dr;
    const float* x[4]; const float* target;
    float hw[4];
    float* stats; float* loss; float* dx[4];
    float gscale; const float* gscale_dev;
    float gamma;
};
enum { SEG_DICE = 0, SEG_BCE = 1, SEG_FOCALDICE = 2, SEG_JACCARD = 3 };
// The 16-byte path of the two Dice kernels: whole float4 per plane and every base 16-byte aligned (with HW % 4 == 0 a plane starts aligned
// where its tensor does).  One function for the kernels and for the dispatchers' query (mtbc_op_kernel_name).
__host__ __device__ inline bool dice_vec16(int HW, const void* a, const void* b, const void* c = nullptr) {
    return (HW & 3) == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}
template <int K> struct SegStride { static constexpr int v = K == SEG_BCE ? 1 : (K == SEG_FOCALDICE ? 4 : 3); };

// softplus(-|x|) = log1p(exp(-|x|)) and exp(-|x|) itself.  The focal term needs five of these per element over 4 x N x H x W elements a step, so
// they are the hardware's v_exp_f32 / v_log_f32 (__expf, __logf) rather than the library's expf / log1pf (a dozen and more instructions each):
// e in (0, 1], so 1 + e in (1, 2] and the absolute error of log(1 + e) stays at ~1e-7 (one rounding of 1 + e, one of the logarithm) -- a relative
// error only where the term itself is below 1e-3 of a unit; __expf's relative error is |arg| * 2^-24 (2e-6 at a logit of 30).
__device__ __forceinline__ float softplus_nabs(float ax, float& e) { e = __expf(-ax); return __logf(1.0f + e); }
__device__ __forceinline__ float bce_logits(float x, float t, float sp) { return (1.0f - t) * x + (fmaxf(-x, 0.f) + sp); }
// focal = m * bce and (want_grad) d focal / d x = -s gamma m (1 - sigmoid(z)) bce + m (p - t), z = -x s; p = sigmoid(x) is returned too
__device__ __forceinline__ float focal_elem(float x, float t, float gamma, float& p, float* grad) {
    float e, ez;
    const float sp = softplus_nabs(fabsf(x), e);
    const float r = 1.0f / (1.0f + e);
    p = x >= 0.f ? r : e * r;
    const float bce = bce_logits(x, t, sp);
    const float s = 2.0f * t - 1.0f, z = -x * s;
    const float spz = softplus_nabs(fabsf(z), ez);          // soft targets: |z| != |x|
    const float m = __expf(gamma * (fminf(z, 0.f) - spz));
    if (grad) {
        const float rz = 1.0f / (1.0f + ez);
        const float nsz = z >= 0.f ? ez * rz : rz;          // 1 - sigmoid(z) = sigmoid(-z)
        *grad = -s * gamma * m * nsz * bce + m * (p - t);
    }
    return m * bce;
}

// one element into the running sums (a0 .. a3: the kind's statistics, in their order)
template <int K>
__device__ __forceinline__ void seg_acc(float x, float t, float gamma, float& a0, float& a1, float& a2, float& a3) {
    if constexpr (K == SEG_BCE) {
        float e;
        const float sp = softplus_nabs(fabsf(x), e);
        a0 += bce_logits(x, t, sp);
    } else if constexpr (K == SEG_FOCALDICE) {
        float pr;
        const float f = focal_elem(x, t, gamma, pr, nullptr);
        a0 = fmaf(pr, t, a0); a1 = fmaf(pr, pr, a1); a2 = fmaf(t, t, a2); a3 += f;
    } else if constexpr (K == SEG_JACCARD) {
        const float pr = sigmoidf_(x);
        a0 = fmaf(pr, t, a0); a1 += pr; a2 += t;
    } else {
        const float pr = sigmoidf_(x);
        a0 = fmaf(pr, t, a0); a1 = fmaf(pr, pr, a1); a2 = fmaf(t, t, a2);
    }
}
template <int K>
__device__ __forceinline__ void seg_acc4(const float4& xv, const float4& tv, float gamma, float& si, float& sp, float& stt, float& a3) {
    if constexpr (K == SEG_DICE) {
        const float px = sigmoidf_(xv.x), py = sigmoidf_(xv.y), pz = sigmoidf_(xv.z), pw = sigmoidf_(xv.w);
        si = fmaf(px, tv.x, si); si = fmaf(py, tv.y, si); si = fmaf(pz, tv.z, si); si = fmaf(pw, tv.w, si);
        sp = fmaf(px, px, sp); sp = fmaf(py, py, sp); sp = fmaf(pz, pz, sp); sp = fmaf(pw, pw, sp);
        stt = fmaf(tv.x, tv.x, stt); stt = fmaf(tv.y, tv.y, stt); stt = fmaf(tv.z, tv.z, stt); stt = fmaf(tv.w, tv.w, stt);
    } else {
        seg_acc<K>(xv.x, tv.x, gamma, si, sp, stt, a3); seg_acc<K>(xv.y, tv.y, gamma, si, sp, stt, a3);
        seg_acc<K>(xv.z, tv.z, gamma, si, sp, stt, a3); seg_acc<K>(xv.w, tv.w, gamma, si, sp, stt, a3);
    }
}

// block = (plane, head): the kind's per-plane sums (kind 0: I = sum p t, P2 = sum p^2, T2 = sum t^2)
template <int K>
__global__ void dice_stats_kernel(const DiceP p) {
    __shared__ float red[32];
    const int plane = blockIdx.x, h = blockIdx.y;
    const float* xs = p.x[h] + (size_t)plane * p.HW;
    const float* ts = p.target + (size_t)plane * p.HW;
    float si = 0.f, sp = 0.f, stt = 0.f, sf = 0.f;
    if (dice_vec16(p.HW, xs, ts)) {
        // 16-byte loads, four rounds in flight per thread (the scalar loop below was one dependent 4-byte round trip per element pair:
        // 40 us for the four 256 x 256 heads of a step -- 128 blocks pulling 512 KB each)
        const float4* x4 = reinterpret_cast<const float4*>(xs);
        const float4* t4 = reinterpret_cast<const float4*>(ts);
        const int n4 = p.HW >> 2, B = blockDim.x;
        int i = threadIdx.x;
        for (; i + 3 * B < n4; i += 4 * B) {
            float4 xv[4], tv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { xv[u] = x4[i + u * B]; tv[u] = t4[i + u * B]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) seg_acc4<K>(xv[u], tv[u], p.gamma, si, sp, stt, sf);
        }
        for (; i < n4; i += B) {
            const float4 xv = x4[i], tv = t4[i];
            seg_acc4<K>(xv, tv, p.gamma, si, sp, stt, sf);
        }
    } else {
        for (int i = threadIdx.x; i < p.HW; i += blockDim.x) seg_acc<K>(xs[i], ts[i], p.gamma, si, sp, stt, sf);
    }
    constexpr int S = SegStride<K>::v;
    si = block_sum(si, red);
    if constexpr (S >= 3) { sp = block_sum(sp, red); stt = block_sum(stt, red); }
    if constexpr (S >= 4) sf = block_sum(sf, red);
    if (threadIdx.x == 0) {
        float* s = p.stats + ((size_t)h * p.planes + plane) * S;
        s[0] = si;
        if constexpr (S >= 3) { s[1] = sp; s[2] = stt; }
        if constexpr (S >= 4) s[3] = sf;
    }
}
// one block: loss[h] = the head's loss (kind 0: mean_plane(1 - (2I+nr)/(P2+T2+dr))); loss[n_heads] = sum_h hw[h] loss[h]
template <int K>
__global__ void dice_finalize_kernel(const DiceP p) {
    __shared__ float red[32];
    constexpr int S = SegStride<K>::v;
    float total = 0.f;
    for (int h = 0; h < p.n_heads; ++h) {
        float s = 0.f;
        for (int i = threadIdx.x; i < p.planes; i += blockDim.x) {
            const float* st = p.stats + ((size_t)h * p.planes + i) * S;
            if constexpr (K == SEG_BCE) s += st[0] / (float)p.HW;
            else if constexpr (K == SEG_JACCARD) s += 1.0f - (2.0f * st[0] + p.nr) / (2.0f * (st[1] + st[2] - st[0]) + p.dr);
            else if constexpr (K == SEG_FOCALDICE) s += (1.0f - (2.0f * st[0] + p.nr) / (st[1] + st[2] + p.dr)) + st[3] / (float)p.HW;
            else s += 1.0f - (2.0f * st[0] + p.nr) / (st[1] + st[2] + p.dr);
        }
        s = block_sum(s, red);
        if constexpr (K != SEG_JACCARD) s = s / (float)p.planes;
        if (threadIdx.x == 0) p.loss[h] = s;
        total += p.hw[h] * s;
    }
    if (threadIdx.x == 0) p.loss[p.n_heads] = total;
}
// one element of the gradient.  den / num: the plane's constants; scale = gscale * hw[h] (/ planes for the means), scale_e = scale / HW
//   kind 0: dx = scale * d f / d p * p (1 - p),  d f / d p = -(2 t (D+dr) - (2I+nr) 2 p) / (D+dr)^2
//   Jaccard: den = 2 (P + T - I) + dr, d den / d p = 2 (1 - t): d f / d p = -(2 t den - num 2 (1 - t)) / den^2
template <int K>
__device__ __forceinline__ float seg_grad(float x, float t, float den, float num, float scale, float scale_e, float gamma) {
    if constexpr (K == SEG_BCE) {
        return scale_e * (sigmoidf_(x) - t);
    } else if constexpr (K == SEG_FOCALDICE) {
        float pr, g;
        focal_elem(x, t, gamma, pr, &g);
        const float dfdp = -(2.0f * t * den - num * 2.0f * pr) / (den * den);
        return scale * dfdp * pr * (1.0f - pr) + scale_e * g;
    } else if constexpr (K == SEG_JACCARD) {
        const float pr = sigmoidf_(x);
        const float dfdp = -(2.0f * t * den - num * 2.0f * (1.0f - t)) / (den * den);
        return scale * dfdp * pr * (1.0f - pr);
    } else {
        const float pr = sigmoidf_(x);
        const float dfdp = -(2.0f * t * den - num * 2.0f * pr) / (den * den);
        return scale * dfdp * pr * (1.0f - pr);
    }
}
template <int K>
__device__ __forceinline__ void seg_plane_consts(const DiceP& p, int h, int plane, float& den, float& num) {
    if constexpr (K == SEG_BCE) {
        den = 1.f; num = 0.f;                               // the gradient of a mean of elementwise terms reads no statistic
    } else {
        const float* st = p.stats + ((size_t)h * p.planes + plane) * SegStride<K>::v;
        if constexpr (K == SEG_JACCARD) den = 2.0f * (st[1] + st[2] - st[0]) + p.dr;
        else den = st[1] + st[2] + p.dr;
        num = 2.0f * st[0] + p.nr;
    }
}
template <int K>
__global__ void dice_bwd_kernel(const DiceP p) {
    const int h = blockIdx.y;
    const size_t total = (size_t)p.planes * p.HW;
    const float scale = K == SEG_JACCARD ? p.gscale * (p.gscale_dev ? *p.gscale_dev : 1.f) * p.hw[h]
                                         : p.gscale * (p.gscale_dev ? *p.gscale_dev : 1.f) * p.hw[h] / (float)p.planes;
    const float scale_e = scale / (float)p.HW;
    if (dice_vec16(p.HW, p.x[h], p.target, p.dx[h])) {
        // four pixels of one plane per thread: 16-byte loads / stores, the plane's constants once per four elements (same formula per element)
        const float4* x4 = reinterpret_cast<const float4*>(p.x[h]);
        const float4* t4 = reinterpret_cast<const float4*>(p.target);
        float4* d4 = reinterpret_cast<float4*>(p.dx[h]);
        const int hw4 = p.HW >> 2;
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (total >> 2); i += (size_t)gridDim.x * blockDim.x) {
            const int plane = (int)(i / hw4);
            float den, num;
            seg_plane_consts<K>(p, h, plane, den, num);
            const float4 xv = x4[i], tv = t4[i];
            const float xe[4] = {xv.x, xv.y, xv.z, xv.w}, te[4] = {tv.x, tv.y, tv.z, tv.w};
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = seg_grad<K>(xe[e], te[e], den, num, scale, scale_e, p.gamma);
            d4[i] = make_float4(o[0], o[1], o[2], o[3]);
        }
        return;
    }
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int plane = i / p.HW;
        float den, num;
        seg_plane_consts<K>(p, h, plane, den, num);
        p.dx[h][i] = seg_grad<K>(p.x[h][i], p.target[i], den, num, scale, scale_e, p.gamma);
    }
}

// ------------------------------------------------------------------ Focal (one block)
struct FocalP {
    int N, C; float alpha, gamma;
    const float* x; const float* t; const float* w; float* loss; float* dx; float gscale; const float* gscale_dev;
};
__global__ void focal_kernel(const FocalP p) {
    __shared__ float red[32];
    float acc = 0.f;
    const float gs = p.gscale * (p.gscale_dev ? *p.gscale_dev : 1.f) / (float)p.N;
    for (int n = threadIdx.x; n < p.N; n += blockDim.x) {
        const float* xs = p.x + (size_t)n * p.C;
        const float* ts = p.t + (size_t)n * p.C;
        if (p.C == 1) {
            // ONE logit = the reference's binary head (n_classes == 2, MTUNetPlusPlus.py:39-41) with torch.nn.BCEWithLogitsLoss
            // (experiment_init.py:241-242): ce = (1 - t) x + softplus(-x), the stable form torch evaluates; alpha = 1, gamma = 0 give
            // exactly its mean; d ce / d x = sigmoid(x) - t.  (`weight`, if given, multiplies the sample's term by w[0].)
            const float x = xs[0], t = ts[0], wc = p.w ? p.w[0] : 1.f;
            const float ce = wc * ((1.0f - t) * x + (fmaxf(-x, 0.f) + log1pf(expf(-fabsf(x)))));
            const float pt = expf(-ce), om = 1.0f - pt;
            const float mod = p.gamma == 0.f ? 1.0f : powf(om, p.gamma);
            acc += p.alpha * mod * ce;
            if (p.dx) {
                const float dmod = p.gamma == 0.f ? 0.f : ((om > 0.f || p.gamma >= 1.f) ? p.gamma * powf(om, p.gamma - 1.0f) : 0.f);
                const float dfdce = p.alpha * (dmod * pt * ce + mod);
                p.dx[n] = gs * dfdce * wc * (1.0f / (1.0f + expf(-x)) - t);
            }
            continue;
        }
        float m = xs[0];
        for (int c = 1; c < p.C; ++c) m = fmaxf(m, xs[c]);
        float se = 0.f;
        for (int c = 0; c < p.C; ++c) se += expf(xs[c] - m);
        const float lse = m + logf(se);
        float ce = 0.f, wt = 0.f;
        for (int c = 0; c < p.C; ++c) {
            const float wc = p.w ? p.w[c] : 1.f;
            ce -= wc * ts[c] * (xs[c] - lse);
            wt += wc * ts[c];
        }
        const float pt = expf(-ce), om = 1.0f - pt;
        const float mod = powf(om, p.gamma);
        acc += p.alpha * mod * ce;
        if (p.dx) {
            // d/dce [alpha (1-pt)^g ce] = alpha ( g (1-pt)^(g-1) pt ce + (1-pt)^g )
            const float dmod = (om > 0.f || p.gamma >= 1.f) ? p.gamma * powf(om, p.gamma - 1.0f) : 0.f;
            const float dfdce = p.alpha * (dmod * pt * ce + mod);
            for (int c = 0; c < p.C; ++c) {
                const float wc = p.w ? p.w[c] : 1.f;
                const float sm = expf(xs[c] - lse);
                p.dx[(size_t)n * p.C + c] = gs * dfdce * (sm * wt - wc * ts[c]);
            }
        }
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) p.loss[0] = acc / (float)p.N;
}

__global__ void loss_mix_kernel(const float* seg, const float* cls, float alpha, float* out4) {
#pragma clang fp contract(off)          // two products and a sum, each rounded, as training_multitask.py:98 forms it in fp32 (contracted, one product
                                        // went unrounded into an fma: the reported loss was 1 ulp off the expression for about every other input)
    const float s = *seg, c = *cls;
    out4[0] = alpha * s + (1.0f - alpha) * c;
    out4[1] = s; out4[2] = c;
    out4[3] = (s != s || c != c) ? 1.f : 0.f;
}

// ------------------------------------------------------------------ softmax over the rows of (N, C), C <= 3 (one block, a thread owns whole rows)
// The row functions are compiled once for host and device (mtbc_softmax_rows_host): exp is written out -- x = n ln 2 + r with ln 2 in two pieces,
// the degree-7 Taylor polynomial on |r| <= ln 2 / 2 (truncation 5e-9 relative), ldexp -- in explicit fused multiply-adds with contraction off,
// so both compilations round the same operations and give the same bits.  x <= 0 here (the row maximum is subtracted first).
__host__ __device__ inline float softmax_exp(float x) {
#pragma clang fp contract(off)
    if (x != x) return x;
    if (x < -104.0f) return 0.f;                               // below half the smallest subnormal (and -inf)
    const float n = rintf(x * 1.44269504088896341f);
    float r = fmaf(-n, 0.693145751953125f, x);                 // ln 2, high 16 bits: n * hi is exact
    r = fmaf(-n, 1.42860682030941723e-6f, r);                  // ... and the rest
    float q = 1.0f / 5040.0f;
    q = fmaf(q, r, 1.0f / 720.0f);
    q = fmaf(q, r, 1.0f / 120.0f);
    q = fmaf(q, r, 1.0f / 24.0f);
    q = fmaf(q, r, 1.0f / 6.0f);
    q = fmaf(q, r, 0.5f);
    q = fmaf(q, r, 1.0f);
    q = fmaf(q, r, 1.0f);
    return ldexpf(q, (int)n);
}
__host__ __device__ inline void softmax_row_fwd(const float* x, float* p, int C) {
#pragma clang fp contract(off)
    float m = x[0];
    for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
    float e[3], s = 0.f;
    for (int c = 0; c < C; ++c) { e[c] = softmax_exp(x[c] - m); s += e[c]; }
    for (int c = 0; c < C; ++c) p[c] = e[c] / s;
}
__host__ __device__ inline void softmax_row_bwd(const float* p, const float* dp, float* dz, int C) {
#pragma clang fp contract(off)
    float s = p[0] * dp[0];
    for (int c = 1; c < C; ++c) s = fmaf(p[c], dp[c], s);
    float o[3];
    for (int c = 0; c < C; ++c) o[c] = p[c] * (dp[c] - s);
    for (int c = 0; c < C; ++c) dz[c] = o[c];                  // dz may alias dp
}
__global__ __launch_bounds__(64) void softmax_rows_kernel(const mtbc_softmax_args a) {
    for (int n = threadIdx.x; n < a.N; n += blockDim.x) {
        const size_t o = (size_t)n * a.C;
        if (a.backward) softmax_row_bwd(a.p + o, a.dp + o, a.dz + o, a.C);
        else softmax_row_fwd(a.x + o, a.p + o, a.C);
    }
}
static int softmax_args_ok(const mtbc_softmax_args* a) {
    if (!a || a->N < 1 || a->C < 1 || a->C > 3) return MTBC_E_BADSHAPE;
    if (!a->p || (a->backward ? (!a->dp || !a->dz) : !a->x)) return MTBC_E_BADARG;
    return MTBC_OK;
}

// ------------------------------------------------------------------ dynamic loss scale (torch.amp.GradScaler's rule on the device)
// The two single-thread halves are plain functions shared by the kernels and by the host-only entry points, so that the rule a machine without a GPU
// tests is the rule the device runs.
__host__ __device__ inline void loss_scale_begin(mtbc_loss_scale_state* s, float* gscale_out, float inv_world, float b1, float b2) {
    if (gscale_out) *gscale_out = s->shard_weight * s->scale;
    const double t1 = (double)(s->t + 1);                      // the step this update would be, if it is applied
    const double bc1 = 1.0 - pow((double)b1, t1);              // as optim_scalars() below: in double, rounded once
    const double bc2 = 1.0 - pow((double)b2, t1);
    s->adam[0] = (float)((double)inv_world / (double)s->scale);
    s->adam[1] = (float)((double)s->lr / bc1);
    s->adam[2] = (float)(1.0 / sqrt(bc2));
}
__host__ __device__ inline void loss_scale_update(mtbc_loss_scale_state* s, double growth, double backoff, int interval) {
    if (s->found_inf) {
        s->scale = (float)((double)s->scale * backoff);
        s->growth_tracker = 0;
        s->skipped += 1;
    } else {
        s->t += 1;
        const int ok = s->growth_tracker + 1;
        if (ok == interval) {
            const float grown = (float)((double)s->scale * growth);
            if (grown - grown == 0.f) s->scale = grown;         // finite: torch._amp_update_scale_ keeps the scale rather than let it become inf
            s->growth_tracker = 0;
        } else {
            s->growth_tracker = ok;
        }
    }
    s->found_inf = 0u;
}
__global__ void loss_scale_begin_kernel(mtbc_loss_scale_state* s, float* gscale_out, float inv_world, float b1, float b2) {
    if (blockIdx.x == 0 && threadIdx.x == 0) loss_scale_begin(s, gscale_out, inv_world, b1, b2);
}
__global__ void loss_scale_update_kernel(mtbc_loss_scale_state* s, double growth, double backoff, int interval) {
    if (blockIdx.x == 0 && threadIdx.x == 0) loss_scale_update(s, growth, backoff, interval);
}
__device__ __forceinline__ unsigned nonfinite_bits(unsigned u) { return (u & 0x7f800000u) == 0x7f800000u; }
__global__ void found_inf_kernel(const float* __restrict__ g, long long n, unsigned* flag) {
    const long long n4 = n >> 2;
    const long long stride = (long long)gridDim.x * blockDim.x;
    unsigned bad = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const uint4 v = reinterpret_cast<const uint4*>(g)[i];
        bad |= nonfinite_bits(v.x) | nonfinite_bits(v.y) | nonfinite_bits(v.z) | nonfinite_bits(v.w);
    }
    for (long long i = (n4 << 2) + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        bad |= nonfinite_bits(reinterpret_cast<const unsigned*>(g)[i]);
    if (bad) atomicOr(flag, 1u);                                // rare (an overflowing step), so no wave reduction in front of it
}

// ------------------------------------------------------------------ Adam, SGD (Nesterov) and AdamW
// One element function for the kernel and for mtbc_optim_step_host: no contraction is left to the compiler (host and device would choose
// differently), every fused operation is an fmaf.  Adam is the AdamW branch with weight_decay 0: decay = (float)(1 - lr 0) = 1 and p * 1.0f is p.
// The branch DEFINES the rule: g' - m as fma(gs, g, -m), the denominator and the last line as one fma each, and v in two forms --
// fma(g', (1-b2) g', b2 v) in the float4 body, the product g' ((1-b2) g') plus the product b2 v in the scalar tail (TAIL: the elements from
// n & ~3 on).  The two forms are how the compiler contracted the kernel Adam had to itself until ABI 203; tests/golden/adam_steps.npz holds its words.
// The rule is therefore position-dependent for v on at most three elements of a buffer (none in training: the flat buffer is a multiple of four).
struct OptimS { float gs, step, inv_bc2_sqrt, decay, omb1, omb2, b2, eps, momentum; int nesterov; };     // step: SGD lr | AdamW lr / (1 - b1^t)
struct OptimP { long long n; float* p; float* g; float* m; float* v; OptimS s; float wd; int kind, zero;
                const float* dyn; const unsigned* skip; const mtbc_loss_scale_state* st; };
template <int KIND, bool TAIL> __host__ __device__ inline void optim1(float& p, float g, float& m, float& v, const OptimS& s) {
#pragma clang fp contract(off)
    const float gp = s.gs * g;
    if (KIND == MTBC_OPT_SGD) {
        m = fmaf(s.momentum, m, gp);
        const float d = s.nesterov ? fmaf(s.momentum, m, gp) : m;
        p = fmaf(-s.step, d, p);
    } else {
        p = p * s.decay;
        m = fmaf(s.omb1, fmaf(s.gs, g, -m), m);
        if (TAIL) v = gp * (s.omb2 * gp) + s.b2 * v; else v = fmaf(gp, s.omb2 * gp, s.b2 * v);
        const float denom = fmaf(sqrtf(v), s.inv_bc2_sqrt, s.eps);
        p = fmaf(-s.step, m / denom, p);
    }
}
__host__ __device__ inline float adamw_decay(float lr, float wd) {
#pragma clang fp contract(off)
    return (float)(1.0 - (double)lr * (double)wd);
}
// the per-step scalars from memory, where the caller put them there: a dynamic loss scale's state first, else the 4 floats of a replayed step
__host__ __device__ inline void optim_resolve(OptimP& a) {
    if (a.st) {
        a.s.gs = a.st->adam[0];
        if (a.kind == MTBC_OPT_SGD) { a.s.step = a.st->lr; }
        else { a.s.step = a.st->adam[1]; a.s.inv_bc2_sqrt = a.st->adam[2]; a.s.decay = adamw_decay(a.st->lr, a.wd); }
    } else if (a.dyn) {
        a.s.gs = a.dyn[0]; a.s.step = a.dyn[1]; a.s.inv_bc2_sqrt = a.dyn[2]; a.s.decay = a.dyn[3];
    }
}
template <int KIND> __device__ __forceinline__ void optim_range(const OptimP& a) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long n4 = a.n >> 2;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 p = reinterpret_cast<float4*>(a.p)[i], g = reinterpret_cast<float4*>(a.g)[i], m = reinterpret_cast<float4*>(a.m)[i];
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (KIND == MTBC_OPT_ADAMW) v = reinterpret_cast<float4*>(a.v)[i];
        optim1<KIND, false>(p.x, g.x, m.x, v.x, a.s); optim1<KIND, false>(p.y, g.y, m.y, v.y, a.s);
        optim1<KIND, false>(p.z, g.z, m.z, v.z, a.s); optim1<KIND, false>(p.w, g.w, m.w, v.w, a.s);
        reinterpret_cast<float4*>(a.p)[i] = p; reinterpret_cast<float4*>(a.m)[i] = m;
        if (KIND == MTBC_OPT_ADAMW) reinterpret_cast<float4*>(a.v)[i] = v;
        if (a.zero) reinterpret_cast<float4*>(a.g)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (long long i = (n4 << 2) + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
        float v = 0.f;
        if (KIND == MTBC_OPT_ADAMW) v = a.v[i];
        optim1<KIND, true>(a.p[i], a.g[i], a.m[i], v, a.s);
        if (KIND == MTBC_OPT_ADAMW) a.v[i] = v;
        if (a.zero) a.g[i] = 0.f;
    }
}
__global__ void optim_kernel(OptimP a) {
    if (a.skip && *a.skip) {                     // dynamic loss scale: a gradient overflowed -> p, m, v are not touched (uniform load, every thread takes the same way)
        const long long stride = (long long)gridDim.x * blockDim.x;
        if (a.zero) for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) a.g[i] = 0.f;
        return;
    }
    optim_resolve(a);                            // uniform loads
    if (a.kind == MTBC_OPT_SGD) optim_range<MTBC_OPT_SGD>(a); else optim_range<MTBC_OPT_ADAMW>(a);
}

// ------------------------------------------------------------------ Dice metric counters (integer, exact)
__global__ void dice_counts_kernel(const float* __restrict__ x, const float* __restrict__ t, long long n,
                                   unsigned long long* cnt) {
    unsigned int tp = 0, fp = 0, fn = 0;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const bool s = sigmoidf_(x[i]) > 0.5f, g = t[i] != 0.f;
        tp += (s && g); fp += (s && !g); fn += (!s && g);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { tp += __shfl_xor(tp, o, 64); fp += __shfl_xor(fp, o, 64); fn += __shfl_xor(fn, o, 64); }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&cnt[0], (unsigned long long)tp); atomicAdd(&cnt[1], (unsigned long long)fp); atomicAdd(&cnt[2], (unsigned long long)fn);
    }
}
__global__ void counts_to_double_kernel(double* out3) {
    if (threadIdx.x < 3) {
        const unsigned long long v = reinterpret_cast<unsigned long long*>(out3)[threadIdx.x];
        out3[threadIdx.x] = (double)v;
    }
}

// ---- the loss launches.  query != NULL: append the launches to *query and return without touching the stream or the device.
constexpr int DICE_FIN_BLOCK = 256, DICE_BWD_BLOCK = 256, DICE_BWD_MAX_BLOCKS = 4096, FOCAL_BLOCK = 256, SOFTMAX_BLOCK = 64;
// What dice_stats_kernel's two loops do on the 16-byte path for n4 float4 a plane and B threads: the unrolled rounds of thread 0 (no thread
// takes more), whether any thread takes a trip of the rest loop, and whether some round or trip is taken by a part of the block only.
struct DiceLoop { int rounds; bool rest, part; };
DiceLoop dice_stats_loop(int n4, int B) {
    DiceLoop s{0, false, false};
    int u0 = 0, r0 = 0;
    for (int t = 0; t < B; ++t) {
        int i = t, u = 0, r = 0;
        for (; i + 3 * B < n4; i += 4 * B) ++u;
        for (; i < n4; i += B) ++r;
        if (t == 0) { u0 = u; r0 = r; }
        s.rest |= r > 0;
        s.part |= u != u0 || r != r0;
    }
    s.rounds = u0;
    return s;
}
void dice_paths(const DiceP& p, bool bwd, char out[5]) {        // per head: v = the 16-byte path, s = the scalar path
    for (int h = 0; h < 4; ++h) out[h] = h >= p.n_heads ? 0 : (dice_vec16(p.HW, p.x[h], p.target, bwd ? p.dx[h] : nullptr) ? 'v' : 's');
    out[4] = 0;
}
template <int K>
int dice_fwd_launch(const DiceP& p, hipStream_t st, OpChoice* query) {
    const int block = p.HW >= 16384 ? 1024 : 256;
    const bool fin_loop = p.planes > DICE_FIN_BLOCK;            // a thread of the finalize block sums more than one plane
    if (query) {
        char paths[5]; dice_paths(p, false, paths);
        const DiceLoop lp = dice_stats_loop(p.HW >> 2, block);
        if (strchr(paths, 'v'))
            query->add("dice_stats_kernel<%d> [threads=%d paths=%s rounds%s%s%s]", K, block, paths, lp.rounds > 1 ? ">1" : lp.rounds ? "=1" : "=0",
                       lp.rest ? " rest" : "", lp.part ? " part" : "");
        else
            query->add("dice_stats_kernel<%d> [threads=%d paths=%s]", K, block, paths);
        query->add(fin_loop ? "dice_finalize_kernel<%d> [planes>256]" : "dice_finalize_kernel<%d>", K);
        return MTBC_OK;
    }
    hipLaunchKernelGGL(dice_stats_kernel<K>, dim3(p.planes, p.n_heads), dim3(block), 0, st, p);
    MTBC_CHECK_LAUNCH();
    hipLaunchKernelGGL(dice_finalize_kernel<K>, dim3(1), dim3(DICE_FIN_BLOCK), 0, st, p);
    MTBC_CHECK_LAUNCH();
    return MTBC_OK;
}
template <int K>
int dice_bwd_launch(const DiceP& p, hipStream_t st, OpChoice* query) {
    const size_t total = (size_t)p.planes * p.HW;
    const size_t want = cdiv64(total, DICE_BWD_BLOCK);
    const bool capped = want > (size_t)DICE_BWD_MAX_BLOCKS;
    const size_t blocks = capped ? (size_t)DICE_BWD_MAX_BLOCKS : want;
    if (query) {          // [loop]: the capped grid has fewer threads than a head has items (float4 on the 16-byte path), so the stride loop takes a second trip
        char paths[5]; dice_paths(p, true, paths);
        bool loop = false;
        for (int h = 0; h < p.n_heads; ++h) loop |= capped && (paths[h] == 'v' ? total >> 2 : total) > blocks * DICE_BWD_BLOCK;
        query->add("dice_bwd_kernel<%d> [paths=%s%s]", K, paths, loop ? " loop" : "");
        return MTBC_OK;
    }
    hipLaunchKernelGGL(dice_bwd_kernel<K>, dim3((unsigned)blocks, p.n_heads), dim3(DICE_BWD_BLOCK), 0, st, p);
    MTBC_CHECK_LAUNCH();
    return MTBC_OK;
}
}  // namespace

// ---------------------------------------------------------------- GAP / Linear: the dispatchers
// query != NULL: validate, append the launches to *query and return without touching the stream or the device (mtbc_op_kernel_name).
int mtbc_i_gap_fwd(const mtbc_gap_args* a, hipStream_t st, OpChoice* query) {
    if (!a || a->N <= 0 || a->C <= 0 || a->H <= 0 || a->W <= 0) return MTBC_E_BADSHAPE;
    if (!a->x || !a->y) return MTBC_E_BADARG;
    if (query) { query->add("gap_fwd_kernel"); return MTBC_OK; }
    const int planes = a->N * a->C;
    hipLaunchKernelGGL(gap_fwd_kernel, dim3(cdiv(planes, 4)), dim3(256), 0, st, a->x, a->y, planes, a->H * a->W);
    MTBC_CHECK_LAUNCH();
    return MTBC_OK;
}
int mtbc_i_gap_bwd(const mtbc_gap_args* a, hipStream_t st, OpChoice* query) {
    if (!a || a->N <= 0 || a->C <= 0 || a->H <= 0 || a->W <= 0) return MTBC_E_BADSHAPE;
    if (!a->dy || !a->dx) return MTBC_E_BADARG;
    if (query) { query->add("gap_bwd_kernel"); return MTBC_OK; }
    const size_t total = (size_t)a->N * a->C * a->H * a->W;
    hipLaunchKernelGGL(gap_bwd_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st, a->dy, a->dx, total, a->H * a->W);
    MTBC_CHECK_LAUNCH();
    return MTBC_OK;
}
// ---- the batch-shared kernels' plans (mtbc.h): by shape alone; the pointers' alignment is checked where they are known
static std::atomic<int> lw_enabled{1};
static bool lw_al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }
static bool lw_shape(const mtbc_linear_args* a) { return lw_enabled.load() != 0 && a->In >= MTBC_LINEAR_WIDE_MIN_IN && (a->In & 3) == 0; }
// forward: S chunks of In (multiples of one wave's 256 floats) so that about 2048 waves run
static void lw_plan_fwd(const mtbc_linear_args* a, int* S, int* kchunk) {
    int s = 2048 / cdiv(a->Out, LW_OT);
    const int smax = cdiv(a->In, 256);
    if (s > smax) s = smax;
    if (s < 1) s = 1;
    *kchunk = cdiv(cdiv(a->In, s), 256) * 256;
    *S = cdiv(a->In, *kchunk);
}
// dx: S ranges of at least 16 outputs so that about 1024 waves run
static void lw_plan_dx(const mtbc_linear_args* a, int* S, int* ochunk) {
    int s = cdiv(1024, cdiv(a->In / 4, 64));
    const int smax = a->Out / 16 > 0 ? a->Out / 16 : 1;
    if (s > smax) s = smax;
    if (s < 1) s = 1;
    *ochunk = cdiv(a->Out, s);
    *S = cdiv(a->Out, *ochunk);
}
static size_t lw_round4(size_t n) { return (n + 3) / 4 * 4; }
extern "C" int mtbc_linear_wide_enable(int32_t on) { return lw_enabled.exchange(on ? 1 : 0); }
extern "C" size_t mtbc_linear_workspace(const mtbc_linear_args* a, int32_t backward) {
    if (!a || a->N <= 0 || a->In <= 0 || a->Out <= 0) return 0;
    int S, chunk;
    if (!backward) {
        if (!lw_shape(a)) return 0;
        lw_plan_fwd(a, &S, &chunk);
        return (size_t)S * a->N * a->Out * sizeof(float);
    }
    size_t floats = a->relu ? (size_t)a->N * a->Out : 0;             // the masked gradient
    if (lw_shape(a) && a->dx) {
        lw_plan_dx(a, &S, &chunk);
        if (S > 1) floats = lw_round4(floats) + (size_t)S * a->N * a->In;      // ... then, 16-byte aligned, the split partials of dx
    }
    return floats * sizeof(float);
}

int mtbc_i_linear_fwd(const mtbc_linear_args* a, hipStream_t st, OpChoice* query) {
    if (!a || a->N <= 0 || a->In <= 0 || a->Out <= 0) return MTBC_E_BADSHAPE;
    if (!a->x || !a->w || !a->y) return MTBC_E_BADARG;
    const bool wide = lw_shape(a) && lw_al16(a->x) && lw_al16(a->w);
    if (wide) {
        int S, kchunk; lw_plan_fwd(a, &S, &kchunk);
        if (!a->workspace || !lw_al16(a->workspace) || a->workspace_bytes < (size_t)S * a->N * a->Out * sizeof(float)) return MTBC_E_WORKSPACE;
        if (query) { query->add("linear_wide_fwd_kernel"); query->add("linear_wide_reduce_kernel"); return MTBC_OK; }
        float* part = reinterpret_cast<float*>(a->workspace);
        hipLaunchKernelGGL(linear_wide_fwd_kernel, dim3(cdiv(a->Out, LW_OT), S), dim3(64), 0, st, a->x, a->w, part, a->N, a->In, a->Out, kchunk);
        MTBC_CHECK_LAUNCH();
        hipLaunchKernelGGL(linear_wide_reduce_kernel, dim3(cdiv(a->N * a->Out, 256)), dim3(256), 0, st, part, a->bias, a->y, S, a->N * a->Out,
                           a->Out, a->relu);
        MTBC_CHECK_LAUNCH();
        return MTBC_OK;
    }
    if (query) { query->add("linear_fwd_kernel"); return MTBC_OK; }
    hipLaunchKernelGGL(linear_fwd_kernel, dim3(cdiv(a->N * a->Out, 4)), dim3(256), 0, st, a->x, a->w, a->bias, a->y, a->N, a->In, a->Out, a->relu);
    MTBC_CHECK_LAUNCH();
    return MTBC_OK;
}
int mtbc_i_linear_bwd(const mtbc_linear_args* a, hipStream_t st, OpChoice* query) {
    if (!a || a->N <= 0 || a->In <= 0 || a->Out <= 0) return MTBC_E_BADSHAPE;
    if (!a->x || !a->w || !a->dy || !a->dw) return MTBC_E_BADARG;
    const float* g = a->dy;
    const bool mask = a->relu != 0, dx = a->dx != nullptr;        // the launches: both paths read these
    if (mask) {
        if (!a->y) return MTBC_E_BADARG;
        if (!a->workspace || a->workspace_bytes < (size_t)a->N * a->Out * sizeof(float)) return MTBC_E_WORKSPACE;
    }
    const bool wide = dx && lw_shape(a) && lw_al16(a->w) && lw_al16(a->dx);
    int S = 1, ochunk = a->Out;
    float* dxpart = nullptr;
    if (wide) {
        lw_plan_dx(a, &S, &ochunk);
        if (S > 1) {
            if (!a->workspace || !lw_al16(a->workspace) || a->workspace_bytes < mtbc_linear_workspace(a, 1)) return MTBC_E_WORKSPACE;
            dxpart = reinterpret_cast<float*>(a->workspace) + lw_round4(mask ? (size_t)a->N * a->Out : 0);
        }
    }
    if (query) {      // [Out>=8] / [N>=8]: the eight-wide unrolled loops of linear_dx_kernel / linear_dw_kernel run
        if (mask) query->add("linear_mask_kernel");
        if (wide) { query->add("linear_wide_dx_kernel"); if (S > 1) query->add("linear_wide_dx_reduce_kernel"); }
        else if (dx) query->add(a->Out >= 8 ? "linear_dx_kernel [Out>=8]" : "linear_dx_kernel");
        query->add(a->N >= 8 ? "linear_dw_kernel [N>=8]" : "linear_dw_kernel");
        return MTBC_OK;
    }
    if (mask) {
        float* gm = reinterpret_cast<float*>(a->workspace);
        hipLaunchKernelGGL(linear_mask_kernel, dim3(cdiv(a->N * a->Out, 256)), dim3(256), 0, st, a->dy, a->y, gm, a->N * a->Out);
        MTBC_CHECK_LAUNCH();
        g = gm;
    }
    if (wide) {
        hipLaunchKernelGGL(linear_wide_dx_kernel, dim3(cdiv(a->In / 4, 64), S), dim3(64), 0, st, g, a->w, S > 1 ? dxpart : a->dx, a->N, a->In,
                           a->Out, ochunk);
        MTBC_CHECK_LAUNCH();
        if (S > 1) {
            const size_t total4 = (size_t)a->N * a->In / 4;
            hipLaunchKernelGGL(linear_wide_dx_reduce_kernel, dim3((unsigned)cdiv64(total4, 256)), dim3(256), 0, st,
                               reinterpret_cast<const float4*>(dxpart), reinterpret_cast<float4*>(a->dx), S, total4);
            MTBC_CHECK_LAUNCH();
        }
    } else if (dx) {
        hipLaunchKernelGGL(linear_dx_kernel, dim3(cdiv(a->N * a->In, 256)), dim3(256), 0, st, g, a->w, a->dx, a->N, a->In, a->Out);
        MTBC_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(linear_dw_kernel, dim3(cdiv(a->Out * a->In, 256)), dim3(256), 0, st, g, a->x, a->dw, a->dbias, a->N, a->In,
                       a->Out, a->accumulate_dw);
    MTBC_CHECK_LAUNCH();
    return MTBC_OK;
}

// ---------------------------------------------------------------- the losses and the softmax: the dispatchers (query: as above)
static int fill_dice(const mtbc_dice_args* a, DiceP* p) {
    if (!a || a->n_heads < 1 || a->n_heads > 4 || a->N <= 0 || a->C <= 0 || a->H <= 0 || a->W <= 0) return MTBC_E_BADSHAPE;
    if (!a->target || !a->stats) return MTBC_E_BADARG;
    if (a->kind < MTBC_SEG_DICE || a->kind > MTBC_SEG_JACCARD) return MTBC_E_UNSUPPORTED;
    p->n_heads = a->n_heads; p->planes = a->N * a->C; p->HW = a->H * a->W; p->nr = a->smooth_nr; p->dr = a->smooth_dr;
    p->target = a->target; p->stats = a->stats; p->loss = a->loss; p->gscale = a->gscale; p->gscale_dev = a->gscale_dev;
    p->gamma = a->focal_gamma;
    for (int h = 0; h < 4; ++h) { p->x[h] = a->x[h]; p->dx[h] = a->dx[h]; p->hw[h] = a->head_weight[h]; }
    for (int h = 0; h < a->n_heads; ++h) if (!a->x[h]) return MTBC_E_BADARG;
    return MTBC_OK;
}
int mtbc_i_dice_fwd(const mtbc_dice_args* a, hipStream_t st, OpChoice* query) {
    DiceP p; int rc = fill_dice(a, &p); if (rc) return rc;
    if (!p.loss) return MTBC_E_BADARG;
    switch (a->kind) {
        case MTBC_SEG_BCE: return dice_fwd_launch<SEG_BCE>(p, st, query);
        case MTBC_SEG_FOCALDICE: return dice_fwd_launch<SEG_FOCALDICE>(p, st, query);
        case MTBC_SEG_JACCARD: return dice_fwd_launch<SEG_JACCARD>(p, st, query);
        default: return dice_fwd_launch<SEG_DICE>(p, st, query);
    }
}
int mtbc_i_dice_bwd(const mtbc_dice_args* a, hipStream_t st, OpChoice* query) {
    DiceP p; int rc = fill_dice(a, &p); if (rc) return rc;
    for (int h = 0; h < a->n_heads; ++h) if (!a->dx[h]) return MTBC_E_BADARG;
    switch (a->kind) {
        case MTBC_SEG_BCE: return dice_bwd_launch<SEG_BCE>(p, st, query);
        case MTBC_SEG_FOCALDICE: return dice_bwd_launch<SEG_FOCALDICE>(p, st, query);
        case MTBC_SEG_JACCARD: return dice_bwd_launch<SEG_JACCARD>(p, st, query);
        default: return dice_bwd_launch<SEG_DICE>(p, st, query);
    }
}
int mtbc_i_focal_fwd_bwd(const mtbc_focal_args* a, hipStream_t st, OpChoice* query) {
    if (!a || a->N <= 0 || a->C <= 0) return MTBC_E_BADSHAPE;
    if (!a->x || !a->target || !a->loss) return MTBC_E_BADARG;
    const int block = FOCAL_BLOCK;                              // one block: from N = block + 1 on a thread owns more than one sample
    if (query) { query->add(a->N > block ? "focal_kernel [N>%d]" : "focal_kernel", block); return MTBC_OK; }
    FocalP p{a->N, a->C, a->alpha, a->gamma, a->x, a->target, a->weight, a->loss, a->dx, a->gscale, a->gscale_dev};
    hipLaunchKernelGGL(focal_kernel, dim3(1), dim3(block), 0, st, p);
    MTBC_CHECK_LAUNCH();
    return MTBC_OK;
}
int mtbc_i_loss_mix(const float* seg, const float* cls, float alpha, float* out4, hipStream_t st, OpChoice* query) {
    if (!seg || !cls || !out4) return MTBC_E_BADARG;
    if (query) { query->add("loss_mix_kernel"); return MTBC_OK; }
    hipLaunchKernelGGL(loss_mix_kernel, dim3(1), dim3(1), 0, st, seg, cls, alpha, out4);
    MTBC_CHECK_LAUNCH();
    return MTBC_OK;
}
int mtbc_i_softmax_rows(const mtbc_softmax_args* a, hipStream_t st, OpChoice* query) {
    const int rc = softmax_args_ok(a);
    if (rc != MTBC_OK) return rc;
    const int block = SOFTMAX_BLOCK;                            // one wave: from N = block + 1 on a thread owns more than one row
    if (query) { query->add(a->N > block ? "softmax_rows_kernel [N>%d]" : "softmax_rows_kernel", block); return MTBC_OK; }
    hipLaunchKernelGGL(softmax_rows_kernel, dim3(1), dim3(block), 0, st, *a);
    MTBC_CHECK_LAUNCH();
    return MTBC_OK;
}

extern "C" {

int mtbc_gap_fwd(const mtbc_gap_args* a, void* stream) { return mtbc_i_gap_fwd(a, (hipStream_t)stream, nullptr); }
int mtbc_gap_bwd(const mtbc_gap_args* a, void* stream) { return mtbc_i_gap_bwd(a, (hipStream_t)stream, nullptr); }
int mtbc_linear_fwd(const mtbc_linear_args* a, void* stream) { return mtbc_i_linear_fwd(a, (hipStream_t)stream, nullptr); }
int mtbc_linear_bwd(const mtbc_linear_args* a, void* stream) { return mtbc_i_linear_bwd(a, (hipStream_t)stream, nullptr); }

int mtbc_dice_fwd(const mtbc_dice_args* a, void* stream) { return mtbc_i_dice_fwd(a, (hipStream_t)stream, nullptr); }
int mtbc_dice_bwd(const mtbc_dice_args* a, void* stream) { return mtbc_i_dice_bwd(a, (hipStream_t)stream, nullptr); }
int mtbc_focal_fwd_bwd(const mtbc_focal_args* a, void* stream) { return mtbc_i_focal_fwd_bwd(a, (hipStream_t)stream, nullptr); }
int mtbc_loss_mix(const float* seg, const float* cls, float alpha, float* out4, void* stream) {
    return mtbc_i_loss_mix(seg, cls, alpha, out4, (hipStream_t)stream, nullptr);
}
int mtbc_softmax_rows(const mtbc_softmax_args* a, void* stream) { return mtbc_i_softmax_rows(a, (hipStream_t)stream, nullptr); }
int mtbc_softmax_rows_host(const mtbc_softmax_args* a) {
    const int rc = softmax_args_ok(a);
    if (rc != MTBC_OK) return rc;
    for (int n = 0; n < a->N; ++n) {
        const size_t o = (size_t)n * a->C;
        if (a->backward) softmax_row_bwd(a->p + o, a->dp + o, a->dz + o, a->C);
        else softmax_row_fwd(a->x + o, a->p + o, a->C);
    }
    return MTBC_OK;
}

static int loss_scale_args_ok(const mtbc_loss_scale_args* a) {
    if (!a || !a->state || (reinterpret_cast<uintptr_t>(a->state) & 3)) return 0;
    return a->growth_interval >= 1 && a->growth_factor > 0.0 && a->backoff_factor > 0.0 && a->inv_world > 0.f;
}
int mtbc_loss_scale_begin(const mtbc_loss_scale_args* a, void* stream) {
    if (!loss_scale_args_ok(a) || !a->gscale_out) return MTBC_E_BADARG;
    hipLaunchKernelGGL(loss_scale_begin_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a->state, a->gscale_out, a->inv_world, a->beta1, a->beta2);
    MTBC_CHECK_LAUNCH();
    return MTBC_OK;
}
int mtbc_loss_scale_check(const mtbc_loss_scale_args* a, void* stream) {
    if (!loss_scale_args_ok(a) || !a->g) return MTBC_E_BADARG;
    if (a->n <= 0) return MTBC_E_BADSHAPE;
    if (reinterpret_cast<uintptr_t>(a->g) & 15) return MTBC_E_UNSUPPORTED;
    long long blocks = cdiv64(a->n / 4 + 1, 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(found_inf_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a->g, (long long)a->n, &a->state->found_inf);
    MTBC_CHECK_LAUNCH();
    return MTBC_OK;
}
int mtbc_loss_scale_update_host(const mtbc_loss_scale_args* a) {
    if (!loss_scale_args_ok(a)) return MTBC_E_BADARG;
    loss_scale_update(a->state, a->growth_factor, a->backoff_factor, a->growth_interval);
    return MTBC_OK;
}
int mtbc_loss_scale_begin_host(const mtbc_loss_scale_args* a) {
    if (!loss_scale_args_ok(a)) return MTBC_E_BADARG;
    loss_scale_begin(a->state, a->gscale_out, a->inv_world, a->beta1, a->beta2);
    return MTBC_OK;
}

// the four per-step scalars, Adam's / AdamW's bias corrections in double on the host, exactly as torch.optim.Adam's scalar path
static void optim_scalars(const mtbc_optim_args* a, float out4[4]) {
    out4[0] = a->grad_scale;
    if (a->kind == MTBC_OPT_SGD) { out4[1] = a->lr; out4[2] = 1.f; out4[3] = 1.f; return; }
    const double bc1 = 1.0 - pow((double)a->beta1, (double)a->step);
    const double bc2 = 1.0 - pow((double)a->beta2, (double)a->step);
    out4[1] = (float)((double)a->lr / bc1);
    out4[2] = (float)(1.0 / sqrt(bc2));
    out4[3] = adamw_decay(a->lr, a->weight_decay);
}
static int optim_kind_ok(const mtbc_optim_args* a) { return a->kind == MTBC_OPT_SGD || a->kind == MTBC_OPT_ADAMW; }
// validation and the kernel's parameter block; `scaled`: under a dynamic loss scale (lr / step / grad_scale are not read)
static int optim_params(const mtbc_optim_args* a, bool scaled, OptimP* p) {
    if (!a || a->n <= 0 || (!scaled && a->step < 1)) return MTBC_E_BADSHAPE;
    if (!optim_kind_ok(a)) return MTBC_E_UNSUPPORTED;
    const bool adamw = a->kind == MTBC_OPT_ADAMW;
    if (!a->p || !a->g || !a->m || (adamw && !a->v)) return MTBC_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(a->p) | reinterpret_cast<uintptr_t>(a->g) | reinterpret_cast<uintptr_t>(a->m) |
         (adamw ? reinterpret_cast<uintptr_t>(a->v) : 0)) & 15)
        return MTBC_E_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(a->dynamic) | reinterpret_cast<uintptr_t>(a->skip) | reinterpret_cast<uintptr_t>(a->scale_state)) & 3) return MTBC_E_BADARG;
    float s4[4] = {0.f, 0.f, 0.f, 0.f};                         // scaled: the kernel takes them from the state
    if (!scaled) optim_scalars(a, s4);
    p->n = a->n; p->p = a->p; p->g = const_cast<float*>(a->g); p->m = a->m; p->v = adamw ? a->v : nullptr;
    p->s.gs = s4[0]; p->s.step = s4[1]; p->s.inv_bc2_sqrt = s4[2]; p->s.decay = s4[3];
    p->s.omb1 = 1.0f - a->beta1; p->s.omb2 = 1.0f - a->beta2; p->s.b2 = a->beta2; p->s.eps = a->eps;
    p->s.momentum = a->momentum; p->s.nesterov = a->nesterov;
    p->wd = a->weight_decay; p->kind = a->kind; p->zero = a->zero_grad;
    p->dyn = a->dynamic; p->skip = a->skip; p->st = a->scale_state;
    return MTBC_OK;
}
static int optim_launch(const OptimP& p, hipStream_t stream) {
    long long blocks = cdiv64(p.n / 4 + 1, 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(optim_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, p);
    MTBC_CHECK_LAUNCH();
    return MTBC_OK;
}
int mtbc_optim_dynamic(const mtbc_optim_args* a, float out4[4]) {
    if (!a || !out4 || a->step < 1 || !optim_kind_ok(a)) return MTBC_E_BADARG;
    optim_scalars(a, out4);
    return MTBC_OK;
}
int mtbc_optim_step(const mtbc_optim_args* a, void* stream) {
    OptimP p;
    const int rc = optim_params(a, a && a->scale_state, &p);
    return rc != MTBC_OK ? rc : optim_launch(p, (hipStream_t)stream);
}
int mtbc_loss_scale_optim(const mtbc_loss_scale_args* a, const mtbc_optim_args* opt, void* stream) {
    if (!loss_scale_args_ok(a)) return MTBC_E_BADARG;
    if (!opt) return MTBC_E_BADARG;
    mtbc_optim_args o = *opt;
    o.dynamic = nullptr; o.skip = &a->state->found_inf; o.scale_state = a->state;
    OptimP p;
    int rc = optim_params(&o, true, &p);
    if (rc == MTBC_OK) rc = optim_launch(p, (hipStream_t)stream);
    if (rc != MTBC_OK) return rc;
    hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a->state, a->growth_factor, a->backoff_factor, a->growth_interval);
    MTBC_CHECK_LAUNCH();
    return MTBC_OK;
}
int mtbc_optim_step_host(const mtbc_optim_args* a) {
    OptimP p;
    const int rc = optim_params(a, a && a->scale_state, &p);
    if (rc != MTBC_OK) return rc;
    if (p.skip && *p.skip) {
        if (p.zero) for (long long i = 0; i < p.n; ++i) p.g[i] = 0.f;
        return MTBC_OK;
    }
    optim_resolve(p);
    const long long body = p.n & ~3LL;                          // the kernel's float4 body; the rest is its scalar tail
    for (long long i = 0; i < p.n; ++i) {
        float v = 0.f;
        if (p.kind == MTBC_OPT_SGD) optim1<MTBC_OPT_SGD, false>(p.p[i], p.g[i], p.m[i], v, p.s);
        else if (i < body) optim1<MTBC_OPT_ADAMW, false>(p.p[i], p.g[i], p.m[i], p.v[i], p.s);
        else optim1<MTBC_OPT_ADAMW, true>(p.p[i], p.g[i], p.m[i], p.v[i], p.s);
        if (p.zero) p.g[i] = 0.f;
    }
    return MTBC_OK;
}

int mtbc_dice_counts(const float* logits, const float* target, int64_t n, double* out3, void* stream) {
    if (!logits || !target || !out3 || n <= 0) return MTBC_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(out3, 0, 3 * sizeof(double), st) != hipSuccess) return MTBC_E_LAUNCH;
    long long blocks = cdiv64(n, 256 * 8);
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(dice_counts_kernel, dim3((unsigned)blocks), dim3(256), 0, st, logits, target, (long long)n,
                       reinterpret_cast<unsigned long long*>(out3));
    MTBC_CHECK_LAUNCH();
    hipLaunchKernelGGL(counts_to_double_kernel, dim3(1), dim3(64), 0, st, out3);
    MTBC_CHECK_LAUNCH();
    return MTBC_OK;
}

}  // extern "C"
