// Per-image metric table of the testing phase (utils/models.py:273-397, metrics.py:26-74, 238-252): confusion counts of the final
// predicted mask, the raw tumour-pixel count, both refining rules, and two set distances, every value an exact integer.
//
// Two launches.  `segm_pack_kernel` turns the logits and the mask into bit planes (one bit per pixel, row-major words and column-major
// words) with __ballot over 64 consecutive pixels and stores per-(image, 64-row block) counts; `segm_dist_kernel` sums those counts,
// applies the rules (the final mask is either the raw one or empty, so its confusion counts follow from the raw ones) and computes
//   hd_rows_sq: max over the rows of one mask of the smallest Hamming distance to a row of the other (what scipy's directed_hausdorff
//               makes of two (H, W) boolean images), both directions;
//   hd_px_sq  : the squared Hausdorff distance of the two pixel sets: for a source pixel (y, x) the squared distance to the target set
//               is min over columns x' of (x - x')^2 + g(y, x')^2 with g the vertical distance to the nearest target pixel of column
//               x', which count-leading / count-trailing zeros give from the column-major words.
// Integer arithmetic only, apart from the shared sigmoid predicate and the class argmax; cross-workgroup results go through plain stores
// (the counts) and integer atomicMax (the distances): bit-reproducible.
#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int SEGM_MAX_DIM = 512;
constexpr int SEGM_PACK_ROWS = 64;       // rows of one pack block = bits of one column-major word
constexpr int SEGM_PACK_THREADS = 1024;  // 16 waves, 4 rows each
constexpr int SEGM_TILE = 16;            // source rows of one distance block (H % 16 == 0)
constexpr int SEGM_DIST_THREADS = 512;
constexpr int SEGM_GROWS = 8;           // rows whose g is in LDS at a time (two passes per tile: keeps two blocks on a CU at 512 x 512)
constexpr int SEGM_GINF = 30000;         // "no target pixel in this column": 30000^2 + 511^2 < 2^31

// Workspace of one image, in 8-byte words: [row S | row G | col S | col G | counts], S = raw prediction, G = ground truth.
//   row plane: word (y, c)  at y * WW + c,  bit b = pixel (y, 64 c + b)
//   col plane: word (x, k)  at x * HB + k,  bit b = pixel (64 k + b, x)
//   counts   : HB x {tp, fp, fn, raw} as uint32 (two words per block)
struct SegmLayout {
    int WW, HB;
    size_t row_words, col_words, rowS, rowG, colS, colG, cnt, image_words;
};
__host__ __device__ inline SegmLayout segm_layout(int H, int W) {
    SegmLayout l;
    l.WW = (W + 63) >> 6; l.HB = (H + 63) >> 6;
    l.row_words = (size_t)H * l.WW; l.col_words = (size_t)W * l.HB;
    l.rowS = 0; l.rowG = l.row_words; l.colS = 2 * l.row_words; l.colG = l.colS + l.col_words;
    l.cnt = l.colG + l.col_words;
    l.image_words = l.cnt + 2 * (size_t)l.HB;
    return l;
}

struct SegmP {
    int N, H, W, n_cls;
    const float* x; const float* t; const float* cls;
    int pixel_threshold, seg_from_class, class_from_seg, normal_class;
    long long* out; u64* ws;
};

// grid (HB, N), 1024 threads: block = 64 rows of one image
__global__ __launch_bounds__(SEGM_PACK_THREADS) void segm_pack_kernel(const SegmP p) {
    __shared__ u64 sS[SEGM_PACK_ROWS][SEGM_MAX_DIM / 64], sG[SEGM_PACK_ROWS][SEGM_MAX_DIM / 64];
    __shared__ unsigned int scnt[4];
    const SegmLayout l = segm_layout(p.H, p.W);
    const int yb = blockIdx.x, img = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64* ws = p.ws + (size_t)img * l.image_words;
    const float* xs = p.x + (size_t)img * p.H * p.W;
    const float* ts = p.t + (size_t)img * p.H * p.W;
    if (threadIdx.x < 4) scnt[threadIdx.x] = 0;
    __syncthreads();
    unsigned int tp = 0, fp = 0, fn = 0, raw = 0;
    for (int r = wave; r < SEGM_PACK_ROWS; r += SEGM_PACK_THREADS / 64) {
        const int y = yb * SEGM_PACK_ROWS + r;
        float xv[SEGM_MAX_DIM / 64], tv[SEGM_MAX_DIM / 64];
#pragma unroll
        for (int c = 0; c < SEGM_MAX_DIM / 64; ++c) {                   // every load of the row in flight before the first ballot
            const int xx = c * 64 + lane;
            const bool in = c < l.WW && y < p.H && xx < p.W;
            xv[c] = in ? xs[(size_t)y * p.W + xx] : -1.f;
            tv[c] = in ? ts[(size_t)y * p.W + xx] : 0.f;
        }
#pragma unroll
        for (int c = 0; c < SEGM_MAX_DIM / 64; ++c) {
            if (c < l.WW) {
                const int xx = c * 64 + lane;
                const bool in = y < p.H && xx < p.W;
                const u64 s = __ballot(in && sigmoidf_(xv[c]) > 0.5f), g = __ballot(in && tv[c] != 0.f);
                tp += __popcll(s & g); fp += __popcll(s & ~g); fn += __popcll(~s & g); raw += __popcll(s);
                if (lane == 0) {
                    sS[r][c] = s; sG[r][c] = g;
                    if (y < p.H) { ws[l.rowS + (size_t)y * l.WW + c] = s; ws[l.rowG + (size_t)y * l.WW + c] = g; }
                }
            }
        }
    }
    if (lane == 0) { atomicAdd(&scnt[0], tp); atomicAdd(&scnt[1], fp); atomicAdd(&scnt[2], fn); atomicAdd(&scnt[3], raw); }
    __syncthreads();
    for (int xx = threadIdx.x; xx < p.W; xx += SEGM_PACK_THREADS) {       // transpose: bit r of the column word = pixel (64 yb + r, xx)
        const int c = xx >> 6, b = xx & 63;
        u64 cs = 0, cg = 0;
#pragma unroll 8
        for (int r = 0; r < SEGM_PACK_ROWS; ++r) { cs |= ((sS[r][c] >> b) & 1ull) << r; cg |= ((sG[r][c] >> b) & 1ull) << r; }
        ws[l.colS + (size_t)xx * l.HB + yb] = cs; ws[l.colG + (size_t)xx * l.HB + yb] = cg;
    }
    if (threadIdx.x == 0) {
        unsigned int* cnt = reinterpret_cast<unsigned int*>(ws + l.cnt) + 4 * yb;
        cnt[0] = scnt[0]; cnt[1] = scnt[1]; cnt[2] = scnt[2]; cnt[3] = scnt[3];
        if (yb == 0) {                                                   // what the distance blocks atomicMax into
            p.out[(size_t)img * MTBC_SEGM_COLS + MTBC_SEGM_HD_ROWS_SQ] = 0;
            p.out[(size_t)img * MTBC_SEGM_COLS + MTBC_SEGM_HD_PX_SQ] = 0;
        }
    }
}

// grid (H / 16, 2, N), 512 threads: block = 16 source rows of one direction (0: prediction -> ground truth, 1: the reverse) of one image.
// dynamic LDS: target row plane | target column plane, stored [k][x] | source rows of the tile | g of 8 rows (uint16)
__global__ __launch_bounds__(SEGM_DIST_THREADS) void segm_dist_kernel(const SegmP p) {
    extern __shared__ u64 lds[];
    __shared__ int smax[2];
    const SegmLayout l = segm_layout(p.H, p.W);
    const int tile = blockIdx.x, dir = blockIdx.y, img = blockIdx.z, tid = threadIdx.x;
    const int H = p.H, W = p.W, WW = l.WW, HB = l.HB;
    const u64* ws = p.ws + (size_t)img * l.image_words;

    // the image's totals and the rules: the same scalars in every thread of every block of the image
    unsigned int tp = 0, fp = 0, fn = 0, raw = 0;
    const unsigned int* cnt = reinterpret_cast<const unsigned int*>(ws + l.cnt);
    for (int b = 0; b < HB; ++b) { tp += cnt[4 * b]; fp += cnt[4 * b + 1]; fn += cnt[4 * b + 2]; raw += cnt[4 * b + 3]; }
    int cls_raw = -1;
    if (p.cls) {
        const float* lg = p.cls + (size_t)img * p.n_cls;
        if (p.n_cls == 1) cls_raw = sigmoidf_(lg[0]) > 0.5f ? 1 : 0;
        else {
            cls_raw = 0;
            float best = lg[0];
            for (int k = 1; k < p.n_cls; ++k) { const float v = lg[k]; if (v > best) { best = v; cls_raw = k; } }
        }
    }
    const bool rules = p.cls && p.n_cls > 1;                                  // the binary head has none (utils/models.py:186-270)
    bool cleared = p.pixel_threshold > 0 && raw <= (unsigned int)p.pixel_threshold;     // images.py:41-55
    cleared = cleared || (rules && p.seg_from_class && cls_raw == p.normal_class);      // utils/models.py:325-332
    const int cls_final = (rules && p.class_from_seg && raw == 0) ? p.normal_class : cls_raw;   // :366-386, on the RAW count
    const unsigned int n_seg = cleared ? 0u : raw, n_gt = tp + fn;
    if (tile == 0 && dir == 0 && tid == 0) {
        long long* o = p.out + (size_t)img * MTBC_SEGM_COLS;
        const long long ftp = cleared ? 0 : tp, ffp = cleared ? 0 : fp, ffn = cleared ? (long long)tp + fn : fn;
        o[MTBC_SEGM_TP] = ftp; o[MTBC_SEGM_FP] = ffp; o[MTBC_SEGM_FN] = ffn;
        o[MTBC_SEGM_TN] = (long long)H * W - ftp - ffp - ffn;
        o[MTBC_SEGM_RAW_PIXELS] = raw; o[MTBC_SEGM_CLS_RAW] = cls_raw; o[MTBC_SEGM_CLS_FINAL] = cls_final;
        if ((n_seg == 0) != (n_gt == 0)) { o[MTBC_SEGM_HD_ROWS_SQ] = -1; o[MTBC_SEGM_HD_PX_SQ] = -1; }     // exactly one empty set
    }
    if (n_seg == 0 || n_gt == 0) return;        // both empty: the zeros of the pack kernel stand; nobody of this image goes on

    const u64* srow = ws + (dir == 0 ? l.rowS : l.rowG);
    const u64* trow = ws + (dir == 0 ? l.rowG : l.rowS);
    const u64* tcol = ws + (dir == 0 ? l.colG : l.colS);
    u64* Lrow = lds;                                      // [H][WW]
    u64* Lcol = Lrow + l.row_words;                       // [HB][W]
    u64* Lsrc = Lcol + l.col_words;                       // [16][WW]
    unsigned short* Lg = reinterpret_cast<unsigned short*>(Lsrc + SEGM_TILE * WW);    // [8][W]
    const int y0 = tile * SEGM_TILE;
    for (int i = tid; i < (int)l.row_words; i += SEGM_DIST_THREADS) Lrow[i] = trow[i];
    for (int i = tid; i < (int)l.col_words; i += SEGM_DIST_THREADS) { const int xx = i / HB, k = i - xx * HB; Lcol[k * W + xx] = tcol[i]; }
    for (int i = tid; i < SEGM_TILE * WW; i += SEGM_DIST_THREADS) Lsrc[i] = srow[(size_t)y0 * WW + i];
    if (tid < 2) smax[tid] = 0;
    __syncthreads();

    // ---- rows: thread = (source row tid / 32, target rows tid % 32 + 32 k)
    {
        const int r = tid >> 5, sub = tid & 31;
        u64 a[SEGM_MAX_DIM / 64];
#pragma unroll
        for (int c = 0; c < SEGM_MAX_DIM / 64; ++c) a[c] = c < WW ? Lsrc[r * WW + c] : 0ull;
        int best = 1 << 30;
        for (int j = sub; j < H; j += 32) {
            int ham = 0;
#pragma unroll
            for (int c = 0; c < SEGM_MAX_DIM / 64; ++c) if (c < WW) ham += __popcll(a[c] ^ Lrow[j * WW + c]);
            best = min(best, ham);
        }
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
        if (sub == 0) atomicMax(&smax[0], best);
    }

    for (int half = 0; half < SEGM_TILE / SEGM_GROWS; ++half) {
    const int r0 = half * SEGM_GROWS;
    // ---- g(y, x'): vertical distance from row y to the nearest target pixel of column x'
    for (int i = tid; i < SEGM_GROWS * W; i += SEGM_DIST_THREADS) {
        const int r = i / W, xx = i - r * W, y = y0 + r0 + r, w = y >> 6, b = y & 63;
        int g = SEGM_GINF;
        {                                                                   // at or above y
            int k = w;
            u64 m = Lcol[k * W + xx] & (~0ull >> (63 - b));
            while (m == 0 && k > 0) { --k; m = Lcol[k * W + xx]; }
            if (m) g = y - (k * 64 + 63 - __clzll((long long)m));
        }
        {                                                                   // at or below y
            int k = w;
            u64 m = Lcol[k * W + xx] & (~0ull << b);
            while (m == 0 && k < HB - 1) { ++k; m = Lcol[k * W + xx]; }
            if (m) g = min(g, k * 64 + __ffsll((unsigned long long)m) - 1 - y);
        }
        Lg[i] = (unsigned short)g;
    }
    __syncthreads();

    // ---- pixels: every source pixel outside the target set scans the columns outwards until (x - x')^2 alone reaches its best;
    //      a pixel whose best has fallen to the block's running maximum cannot raise it and stops (the result does not depend on that)
    for (int i = tid; i < SEGM_GROWS * W; i += SEGM_DIST_THREADS) {
        const int r = i / W, xx = i - r * W;
        if (!((Lsrc[(r0 + r) * WW + (xx >> 6)] >> (xx & 63)) & 1ull)) continue;
        const unsigned short* gr = Lg + r * W;
        const int g0 = gr[xx];
        if (g0 == 0) continue;                                               // the pixel is in the target set
        int best = g0 * g0;
        for (int d = 1; d < W; ++d) {
            const int dd = d * d;
            if (dd >= best) break;
            const int xl = xx - d, xr = xx + d;
            if (xl < 0 && xr >= W) break;
            if (xl >= 0) { const int g = gr[xl]; best = min(best, dd + g * g); }
            if (xr < W) { const int g = gr[xr]; best = min(best, dd + g * g); }
            if (best <= *(volatile int*)&smax[1]) break;
        }
        if (best > *(volatile int*)&smax[1]) atomicMax(&smax[1], best);
    }
    __syncthreads();
    }
    if (tid == 0) {
        unsigned long long* o = reinterpret_cast<unsigned long long*>(p.out + (size_t)img * MTBC_SEGM_COLS);
        atomicMax(&o[MTBC_SEGM_HD_ROWS_SQ], (unsigned long long)smax[0]);
        atomicMax(&o[MTBC_SEGM_HD_PX_SQ], (unsigned long long)smax[1]);
    }
}

size_t segm_dist_lds_bytes(int H, int W) {
    const SegmLayout l = segm_layout(H, W);
    return (l.row_words + l.col_words + (size_t)SEGM_TILE * l.WW) * sizeof(u64) + (size_t)SEGM_GROWS * W * sizeof(unsigned short);
}

int segm_check_shape(const mtbc_seg_metrics_args* a) {
    if (!a) return MTBC_E_BADARG;
    if (a->N <= 0 || a->H < 16 || a->W < 16 || a->H > SEGM_MAX_DIM || a->W > SEGM_MAX_DIM || (a->H & 15) || (a->W & 15)) return MTBC_E_BADSHAPE;
    if ((int64_t)a->N > 65535) return MTBC_E_BADSHAPE;           // the image index is a grid dimension
    return MTBC_OK;
}

}  // namespace

extern "C" {

size_t mtbc_seg_metrics_workspace_size(const mtbc_seg_metrics_args* a) {
    if (segm_check_shape(a) != MTBC_OK) return 0;
    return (size_t)a->N * segm_layout(a->H, a->W).image_words * sizeof(u64);
}

int mtbc_seg_metrics(const mtbc_seg_metrics_args* a, void* stream) {
    const int rc = segm_check_shape(a);
    if (rc != MTBC_OK) return rc;
    if (!a->seg_logits || !a->target || !a->out || !a->workspace) return MTBC_E_BADARG;
    if (a->cls_logits && (a->n_cls < 1 || a->n_cls > 64)) return MTBC_E_BADARG;
    if (a->pixel_threshold < 0) return MTBC_E_BADARG;
    if (((uintptr_t)a->workspace & 7) || ((uintptr_t)a->out & 7)) return MTBC_E_BADARG;
    if (a->workspace_bytes < mtbc_seg_metrics_workspace_size(a)) return MTBC_E_WORKSPACE;
    SegmP p;
    p.N = a->N; p.H = a->H; p.W = a->W; p.n_cls = a->cls_logits ? a->n_cls : 0;
    p.x = a->seg_logits; p.t = a->target; p.cls = a->cls_logits;
    p.pixel_threshold = a->pixel_threshold; p.seg_from_class = a->seg_from_class; p.class_from_seg = a->class_from_seg;
    p.normal_class = a->normal_class;
    p.out = reinterpret_cast<long long*>(a->out); p.ws = static_cast<u64*>(a->workspace);
    hipStream_t st = (hipStream_t)stream;
    const SegmLayout l = segm_layout(a->H, a->W);
    hipLaunchKernelGGL(segm_pack_kernel, dim3(l.HB, a->N), dim3(SEGM_PACK_THREADS), 0, st, p);
    MTBC_CHECK_LAUNCH();
    const size_t lds = segm_dist_lds_bytes(a->H, a->W);            // 73 KB at 512 x 512: two blocks per CU
    MTBC_ENSURE_DYN_LDS(segm_dist_kernel, (int)segm_dist_lds_bytes(SEGM_MAX_DIM, SEGM_MAX_DIM));
    hipLaunchKernelGGL(segm_dist_kernel, dim3(a->H / SEGM_TILE, 2, a->N), dim3(SEGM_DIST_THREADS), lds, st, p);
    MTBC_CHECK_LAUNCH();
    return MTBC_OK;
}

}  // extern "C"
