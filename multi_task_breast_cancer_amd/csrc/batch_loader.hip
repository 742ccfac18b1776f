// Batch assembly from a device-resident uint8 dataset (the training-epoch side): ONE launch goes from a
// device index array to the step's filled fp32 input buffers.
//
// The reference keeps the whole dataset in RAM as uint8 (BUSI_dataset.py:47-92) and builds each item on the CPU (:97-158): float
// image, float mask, the intensity variants of `data.augmentation` (:123-139, each a pure function of the pixel value = a 256-entry
// look-up table), then ONE joint flip / rotation of cat([mask, image] + extras) (:153-158) and, in the training loop, the one-hot label
// (training_multitask.py:84).  Here sample n of the batch is store row index[n]; every plane of a sample takes the SAME source pixel
// (flip_rotate_src of common.h, shared with augment.hip) and is 0 outside the rotated frame -- the LUT planes too, as in the reference,
// which rotates the already-brightened plane with zero fill.
//
// HBM-write-bound: (2 + K) * 4 bytes written per pixel against <= 2 bytes read.  A thread owns 4 consecutive output pixels of one
// sample and writes one 16-byte store per plane; the identity path (params == NULL: validation / test) reads its source as one 4-byte
// word, the rotated path gathers bytes (the whole store sits in L2 / the memory-side cache).  W % 4 != 0 or an unaligned buffer takes
// the scalar instance of the same kernel.  The LUTs are staged in LDS once per block.  The class target of sample n is written by the
// thread that holds the sample's pixel 0.  No atomics, no workspace, every output element written exactly once by this launch.
#include "common.h"

namespace {

struct BatchP {
    int M, N, H, W, K, n_onehot;
    const uint8_t* images;
    const uint8_t* masks;
    const int32_t* labels;
    const int32_t* index;
    const float* params;          // (N, 4) {cos a, sin a, flip_h, flip_v} or nullptr = identity
    const uint8_t* luts;          // (K, 256)
    float* out_image;             // (N, 1 + K, H, W)
    float* out_mask;              // (N, 1, H, W)
    float* out_target;            // (N, 3) one-hot, or (N, 1) float label when n_onehot == 0
};

constexpr int BATCH_BLOCK = 256;
constexpr int BATCH_MAX_LUTS = MTBC_BATCH_MAX_LUTS;

// VEC: W % 4 == 0 and 16-byte aligned outputs / 4-byte aligned stores -- the 4 pixels of a thread lie in one row
template <bool VEC>
__global__ __launch_bounds__(BATCH_BLOCK) void batch_assemble_kernel(const BatchP p) {
    __shared__ uint8_t lut[BATCH_MAX_LUTS * 256];
    for (int i = threadIdx.x; i < p.K * 256; i += BATCH_BLOCK) lut[i] = p.luts[i];
    __syncthreads();

    const long long HW = (long long)p.H * p.W;
    const long long G = (HW + 3) / 4;                         // 4-pixel groups per sample
    const long long total = (long long)p.N * G;
    const int C = 1 + p.K;
    for (long long t = (long long)blockIdx.x * BATCH_BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * BATCH_BLOCK) {
        const int n = (int)(t / G);
        const long long pix0 = 4 * (t % G);
        const int idx = p.index[n];
        const bool ok = idx >= 0 && idx < p.M;              // an index outside the store never touches it: the sample is written as zeros
        const size_t row = (size_t)(ok ? idx : 0) * (size_t)HW;
        const uint8_t* si = p.images + row;
        const uint8_t* sm = p.masks + row;

        uint32_t raw[4], msk[4];
        bool take[4];
        if (!p.params) {
            if (VEC) {
                const uint32_t wi = ok ? *reinterpret_cast<const uint32_t*>(si + pix0) : 0u;
                const uint32_t wm = ok ? *reinterpret_cast<const uint32_t*>(sm + pix0) : 0u;
#pragma unroll
                for (int j = 0; j < 4; ++j) { raw[j] = (wi >> (8 * j)) & 255u; msk[j] = (wm >> (8 * j)) & 255u; take[j] = ok; }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    take[j] = ok && pix0 + j < HW;
                    raw[j] = take[j] ? si[pix0 + j] : 0u;
                    msk[j] = take[j] ? sm[pix0 + j] : 0u;
                }
            }
        } else {
            const float ca = p.params[4 * n], sa = p.params[4 * n + 1];
            const bool fh = p.params[4 * n + 2] != 0.f, fv = p.params[4 * n + 3] != 0.f;
            const int y0 = (int)(pix0 / p.W), x0 = (int)(pix0 % p.W);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int x = x0 + j, y = y0;
                if (!VEC) { const long long pix = pix0 + j; y = (int)(pix / p.W); x = (int)(pix % p.W); }
                int xs, ys;
                const bool inb = flip_rotate_src(x, y, p.H, p.W, ca, sa, fh, fv, xs, ys);
                take[j] = inb && ok && (VEC || pix0 + j < HW);
                const size_t so = (size_t)ys * p.W + xs;
                raw[j] = take[j] ? si[so] : 0u;
                msk[j] = take[j] ? sm[so] : 0u;
            }
        }

        float* om = p.out_mask + (size_t)n * HW + pix0;
        float* oi = p.out_image + (size_t)n * C * HW + pix0;
        if (VEC) {
            *reinterpret_cast<f32x4*>(om) = f32x4{(float)msk[0], (float)msk[1], (float)msk[2], (float)msk[3]};
            *reinterpret_cast<f32x4*>(oi) = f32x4{(float)raw[0], (float)raw[1], (float)raw[2], (float)raw[3]};
#pragma unroll
            for (int k = 0; k < BATCH_MAX_LUTS; ++k) {
                if (k < p.K) {
                    f32x4 v;
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = take[j] ? (float)lut[k * 256 + raw[j]] : 0.f;
                    *reinterpret_cast<f32x4*>(oi + (size_t)(k + 1) * HW) = v;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (pix0 + j < HW) {
                    om[j] = (float)msk[j];
                    oi[j] = (float)raw[j];
#pragma unroll
                    for (int k = 0; k < BATCH_MAX_LUTS; ++k)
                        if (k < p.K) oi[(size_t)(k + 1) * HW + j] = take[j] ? (float)lut[k * 256 + raw[j]] : 0.f;
                }
            }
        }
        if (pix0 == 0) {                                      // this thread holds pixel 0 of sample n: it writes the sample's class target
            const int lab = ok ? p.labels[idx] : -1;
            if (p.n_onehot == 0) {
                p.out_target[n] = ok ? (float)lab : 0.f;
            } else {
                for (int c = 0; c < p.n_onehot; ++c) p.out_target[(size_t)n * p.n_onehot + c] = lab == c ? 1.f : 0.f;
            }
        }
    }
}

// ---- the same launch with E stored planes per image (mtbc_batch_assemble_planes): the spatial variants of `data.augmentation` (CLAHE,
// SOBEL) are data the caller computed once per image, kept as uint8 stores (E, M, H, W) next to the image store.  A stored plane goes the
// image plane's way -- the same store row, the same source pixel, 0 outside the rotated frame -- into channels 1 .. E, in front of the LUT
// channels.  (2 + E + K) * 4 bytes written per pixel against <= 2 + E read.  A kernel of its own: batch_assemble_kernel above keeps its
// instances, and with E == 0 this one writes the same words.
constexpr int BATCH_MAX_PLANES = MTBC_BATCH_MAX_PLANES;

struct BatchPlanesP {
    BatchP b;                     // out_image is (N, 1 + E + K, H, W)
    int E;
    const uint8_t* planes;        // (E, M, H, W)
};

// VEC: as above, and `planes` / M * H * W 4-byte aligned -- every plane's row starts on a word
template <bool VEC>
__global__ __launch_bounds__(BATCH_BLOCK) void batch_assemble_planes_kernel(const BatchPlanesP q) {
    const BatchP& p = q.b;
    __shared__ uint8_t lut[BATCH_MAX_LUTS * 256];
    for (int i = threadIdx.x; i < p.K * 256; i += BATCH_BLOCK) lut[i] = p.luts[i];
    __syncthreads();

    const long long HW = (long long)p.H * p.W;
    const long long G = (HW + 3) / 4;                         // 4-pixel groups per sample
    const long long total = (long long)p.N * G;
    const size_t store = (size_t)p.M * (size_t)HW;            // one stored plane of every image
    const int C = 1 + q.E + p.K;
    for (long long t = (long long)blockIdx.x * BATCH_BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * BATCH_BLOCK) {
        const int n = (int)(t / G);
        const long long pix0 = 4 * (t % G);
        const int idx = p.index[n];
        const bool ok = idx >= 0 && idx < p.M;              // an index outside the store never touches it: the sample is written as zeros
        const size_t row = (size_t)(ok ? idx : 0) * (size_t)HW;
        const uint8_t* si = p.images + row;
        const uint8_t* sm = p.masks + row;
        const uint8_t* sp = q.planes + row;                  // plane e of this row: sp + e * store (never formed with E == 0)

        // (the loops over the planes and the LUTs run to their compile-time maxima with the count tested inside: a register array
        //  indexed by a run-time trip count would go to a private segment)
        uint32_t raw[4], msk[4], ext[BATCH_MAX_PLANES][4];
        bool take[4];
        if (!p.params) {
            if (VEC) {
                const uint32_t wi = ok ? *reinterpret_cast<const uint32_t*>(si + pix0) : 0u;
                const uint32_t wm = ok ? *reinterpret_cast<const uint32_t*>(sm + pix0) : 0u;
#pragma unroll
                for (int j = 0; j < 4; ++j) { raw[j] = (wi >> (8 * j)) & 255u; msk[j] = (wm >> (8 * j)) & 255u; take[j] = ok; }
#pragma unroll
                for (int e = 0; e < BATCH_MAX_PLANES; ++e) {
                    const uint32_t we = (e < q.E && ok) ? *reinterpret_cast<const uint32_t*>(sp + (size_t)e * store + pix0) : 0u;
#pragma unroll
                    for (int j = 0; j < 4; ++j) ext[e][j] = (we >> (8 * j)) & 255u;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    take[j] = ok && pix0 + j < HW;
                    raw[j] = take[j] ? si[pix0 + j] : 0u;
                    msk[j] = take[j] ? sm[pix0 + j] : 0u;
#pragma unroll
                    for (int e = 0; e < BATCH_MAX_PLANES; ++e) ext[e][j] = (e < q.E && take[j]) ? sp[(size_t)e * store + pix0 + j] : 0u;
                }
            }
        } else {
            const float ca = p.params[4 * n], sa = p.params[4 * n + 1];
            const bool fh = p.params[4 * n + 2] != 0.f, fv = p.params[4 * n + 3] != 0.f;
            const int y0 = (int)(pix0 / p.W), x0 = (int)(pix0 % p.W);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int x = x0 + j, y = y0;
                if (!VEC) { const long long pix = pix0 + j; y = (int)(pix / p.W); x = (int)(pix % p.W); }
                int xs, ys;
                const bool inb = flip_rotate_src(x, y, p.H, p.W, ca, sa, fh, fv, xs, ys);
                take[j] = inb && ok && (VEC || pix0 + j < HW);
                const size_t so = (size_t)ys * p.W + xs;
                raw[j] = take[j] ? si[so] : 0u;
                msk[j] = take[j] ? sm[so] : 0u;
#pragma unroll
                for (int e = 0; e < BATCH_MAX_PLANES; ++e) ext[e][j] = (e < q.E && take[j]) ? sp[(size_t)e * store + so] : 0u;
            }
        }

        float* om = p.out_mask + (size_t)n * HW + pix0;
        float* oi = p.out_image + (size_t)n * C * HW + pix0;
        float* ol = oi + (size_t)q.E * HW;                    // LUT channel k at ol + (k + 1) * HW
        if (VEC) {
            *reinterpret_cast<f32x4*>(om) = f32x4{(float)msk[0], (float)msk[1], (float)msk[2], (float)msk[3]};
            *reinterpret_cast<f32x4*>(oi) = f32x4{(float)raw[0], (float)raw[1], (float)raw[2], (float)raw[3]};
#pragma unroll
            for (int e = 0; e < BATCH_MAX_PLANES; ++e)
                if (e < q.E)
                    *reinterpret_cast<f32x4*>(oi + (size_t)(e + 1) * HW) = f32x4{(float)ext[e][0], (float)ext[e][1], (float)ext[e][2], (float)ext[e][3]};
#pragma unroll
            for (int k = 0; k < BATCH_MAX_LUTS; ++k) {
                if (k < p.K) {
                    f32x4 v;
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = take[j] ? (float)lut[k * 256 + raw[j]] : 0.f;
                    *reinterpret_cast<f32x4*>(ol + (size_t)(k + 1) * HW) = v;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (pix0 + j < HW) {
                    om[j] = (float)msk[j];
                    oi[j] = (float)raw[j];
#pragma unroll
                    for (int e = 0; e < BATCH_MAX_PLANES; ++e)
                        if (e < q.E) oi[(size_t)(e + 1) * HW + j] = (float)ext[e][j];
#pragma unroll
                    for (int k = 0; k < BATCH_MAX_LUTS; ++k)
                        if (k < p.K) ol[(size_t)(k + 1) * HW + j] = take[j] ? (float)lut[k * 256 + raw[j]] : 0.f;
                }
            }
        }
        if (pix0 == 0) {                                      // this thread holds pixel 0 of sample n: it writes the sample's class target
            const int lab = ok ? p.labels[idx] : -1;
            if (p.n_onehot == 0) {
                p.out_target[n] = ok ? (float)lab : 0.f;
            } else {
                for (int c = 0; c < p.n_onehot; ++c) p.out_target[(size_t)n * p.n_onehot + c] = lab == c ? 1.f : 0.f;
            }
        }
    }
}

inline bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

}  // namespace

extern "C" int mtbc_batch_assemble(const mtbc_batch_args* a, void* stream) {
    if (!a) return MTBC_E_BADARG;
    if (a->M <= 0 || a->N <= 0 || a->H <= 0 || a->W <= 0 || a->K < 0 || a->K > MTBC_BATCH_MAX_LUTS) return MTBC_E_BADSHAPE;
    if (a->n_onehot != 0 && a->n_onehot != 3) return MTBC_E_BADSHAPE;
    if (!a->images || !a->masks || !a->labels || !a->index || !a->out_image || !a->out_mask || !a->out_target) return MTBC_E_BADARG;
    if (a->K > 0 && !a->luts) return MTBC_E_BADARG;
    const size_t HW = (size_t)a->H * a->W, store = (size_t)a->M * HW;
    const size_t n_img = (size_t)a->N * (1 + a->K) * HW * 4, n_msk = (size_t)a->N * HW * 4, n_tgt = (size_t)a->N * (a->n_onehot ? a->n_onehot : 1) * 4;
    const struct { const void* p; size_t n; } outs[3] = {{a->out_image, n_img}, {a->out_mask, n_msk}, {a->out_target, n_tgt}};
    const struct { const void* p; size_t n; } ins[6] = {{a->images, store}, {a->masks, store}, {a->labels, (size_t)a->M * 4}, {a->index, (size_t)a->N * 4},
                                                        {a->params, a->params ? (size_t)a->N * 16 : 0}, {a->luts, (size_t)a->K * 256}};
    for (int i = 0; i < 3; ++i) {
        for (int j = i + 1; j < 3; ++j)
            if (overlaps(outs[i].p, outs[i].n, outs[j].p, outs[j].n)) return MTBC_E_BADARG;
        for (int j = 0; j < 6; ++j)
            if (ins[j].n && overlaps(outs[i].p, outs[i].n, ins[j].p, ins[j].n)) return MTBC_E_BADARG;
    }
    BatchP p{a->M, a->N, a->H, a->W, a->K, a->n_onehot, a->images, a->masks, a->labels, a->index, a->params, a->luts,
             a->out_image, a->out_mask, a->out_target};
    const bool vec = a->W % 4 == 0 && (uintptr_t)a->out_image % 16 == 0 && (uintptr_t)a->out_mask % 16 == 0 &&
                     (uintptr_t)a->images % 4 == 0 && (uintptr_t)a->masks % 4 == 0;
    const long long total = (long long)a->N * (long long)((HW + 3) / 4);
    // memory-bound: at most 8 blocks per CU's worth of blocks, the rest of the work is grid-strided
    const unsigned grid = (unsigned)(cdiv64(total, BATCH_BLOCK) < 2048 ? cdiv64(total, BATCH_BLOCK) : 2048);
    if (vec) hipLaunchKernelGGL(batch_assemble_kernel<true>, dim3(grid), dim3(BATCH_BLOCK), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(batch_assemble_kernel<false>, dim3(grid), dim3(BATCH_BLOCK), 0, (hipStream_t)stream, p);
    MTBC_CHECK_LAUNCH();
    return MTBC_OK;
}

extern "C" int mtbc_batch_assemble_planes(const mtbc_batch_planes_args* a, void* stream) {
    if (!a) return MTBC_E_BADARG;
    if (a->M <= 0 || a->N <= 0 || a->H <= 0 || a->W <= 0 || a->K < 0 || a->K > MTBC_BATCH_MAX_LUTS) return MTBC_E_BADSHAPE;
    if (a->n_onehot != 0 && a->n_onehot != 3) return MTBC_E_BADSHAPE;
    if (a->E < 0 || a->E > MTBC_BATCH_MAX_PLANES) return MTBC_E_BADSHAPE;
    if (!a->images || !a->masks || !a->labels || !a->index || !a->out_image || !a->out_mask || !a->out_target) return MTBC_E_BADARG;
    if (a->K > 0 && !a->luts) return MTBC_E_BADARG;
    if (a->E > 0 && !a->planes) return MTBC_E_BADARG;
    const size_t HW = (size_t)a->H * a->W, store = (size_t)a->M * HW;
    const size_t n_img = (size_t)a->N * (1 + a->E + a->K) * HW * 4, n_msk = (size_t)a->N * HW * 4, n_tgt = (size_t)a->N * (a->n_onehot ? a->n_onehot : 1) * 4;
    const struct { const void* p; size_t n; } outs[3] = {{a->out_image, n_img}, {a->out_mask, n_msk}, {a->out_target, n_tgt}};
    const struct { const void* p; size_t n; } ins[7] = {{a->images, store}, {a->masks, store}, {a->labels, (size_t)a->M * 4}, {a->index, (size_t)a->N * 4},
                                                        {a->params, a->params ? (size_t)a->N * 16 : 0}, {a->luts, (size_t)a->K * 256},
                                                        {a->planes, (size_t)a->E * store}};
    for (int i = 0; i < 3; ++i) {
        for (int j = i + 1; j < 3; ++j)
            if (overlaps(outs[i].p, outs[i].n, outs[j].p, outs[j].n)) return MTBC_E_BADARG;
        for (int j = 0; j < 7; ++j)
            if (ins[j].n && overlaps(outs[i].p, outs[i].n, ins[j].p, ins[j].n)) return MTBC_E_BADARG;
    }
    BatchPlanesP q{{a->M, a->N, a->H, a->W, a->K, a->n_onehot, a->images, a->masks, a->labels, a->index, a->params, a->luts,
                    a->out_image, a->out_mask, a->out_target}, a->E, a->planes};
    const bool vec = a->W % 4 == 0 && (uintptr_t)a->out_image % 16 == 0 && (uintptr_t)a->out_mask % 16 == 0 &&
                     (uintptr_t)a->images % 4 == 0 && (uintptr_t)a->masks % 4 == 0 &&
                     (a->E == 0 || ((uintptr_t)a->planes % 4 == 0 && store % 4 == 0));
    const long long total = (long long)a->N * (long long)((HW + 3) / 4);
    const unsigned grid = (unsigned)(cdiv64(total, BATCH_BLOCK) < 2048 ? cdiv64(total, BATCH_BLOCK) : 2048);
    if (vec) hipLaunchKernelGGL(batch_assemble_planes_kernel<true>, dim3(grid), dim3(BATCH_BLOCK), 0, (hipStream_t)stream, q);
    else hipLaunchKernelGGL(batch_assemble_planes_kernel<false>, dim3(grid), dim3(BATCH_BLOCK), 0, (hipStream_t)stream, q);
    MTBC_CHECK_LAUNCH();
    return MTBC_OK;
}
