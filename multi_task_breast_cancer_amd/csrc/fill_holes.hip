// Hole filling of the predicted mask in the segmentation driver's testing phase (utils/models.py:39-100, fill_holes=True):
// scipy.ndimage.binary_fill_holes with its default structure.  foreground = sigmoidf_(x) > .5f (common.h: the predicate of the Dice counters,
// a NaN is not foreground); a non-foreground ("free") pixel is reached when it lies on the border or is 4-adjacent to a reached free pixel;
// the output is the complement of the reached set.
//
// One workgroup per image.  Two bit planes in LDS, `free` and `reached`, one bit per pixel in 32-bit words, row (y) at y * stride with
// stride = words per row | 1 (odd: a thread per row walks its words without a bank conflict against its neighbours): 2 x 34 KB at 512 x 512,
// dynamic LDS.  A pass is four directional sweeps of r[i] |= r[i-1] & free[i]:
//   rows     one thread per row: left -> right then right -> left, bit-parallel inside a word (a 5-step prefix fill) with a carry between
//            words; the border enters as a carry of 1
//   columns  one thread per word column (32 pixel columns at once): top -> bottom then bottom -> top, the border as an all-ones row
// with a workgroup barrier between the two halves and behind the pass; a pass that set no bit ends the loop (a vote through an LDS word).
// Every non-final pass sets at least one of H * W bits, so the loop is a `for` bounded by H * W + 1; reaching the bound sets *error.
// No global atomics, nothing between workgroups: the result is deterministic.
//
// fh_fill and its sweeps are the ONE body for the kernel and for mtbc_fill_holes_host: the host instantiation runs it as thread 0 of 1 with
// barriers that do nothing, so the host function states the kernel's arithmetic (the predicate is common.h's, compiled for both).
#include "common.h"

namespace {

constexpr int FH_MAX_DIM = 512;
constexpr int FH_THREADS = 512;

__host__ __device__ inline int fh_words(int W) { return (W + 31) >> 5; }
__host__ __device__ inline int fh_stride(int W) { return fh_words(W) | 1; }
__host__ __device__ inline size_t fh_plane_words(int H, int W) { return (size_t)H * fh_stride(W); }

// reached bits of one word after a sweep towards HIGHER bit indices: seeds g (a subset of f), free bits f, carry into bit 0
__host__ __device__ inline uint32_t fh_fill_up(uint32_t g, uint32_t f, uint32_t carry) {
    g |= f & carry;
    g |= f & (g << 1); f &= f << 1;
    g |= f & (g << 2); f &= f << 2;
    g |= f & (g << 4); f &= f << 4;
    g |= f & (g << 8); f &= f << 8;
    g |= f & (g << 16);
    return g;
}
// ... towards LOWER bit indices, carry into bit 31
__host__ __device__ inline uint32_t fh_fill_down(uint32_t g, uint32_t f, uint32_t carry) {
    g |= f & (carry << 31);
    g |= f & (g >> 1); f &= f >> 1;
    g |= f & (g >> 2); f &= f >> 2;
    g |= f & (g >> 4); f &= f >> 4;
    g |= f & (g >> 8); f &= f >> 8;
    g |= f & (g >> 16);
    return g;
}

struct HostSync { inline void operator()() const {} };
struct DevSync { __device__ inline void operator()() const { __syncthreads(); } };

// rows t0, t0 + nt, ...: both horizontal sweeps; true when a bit was set
__host__ __device__ inline bool fh_sweep_rows(const uint32_t* fr, uint32_t* re, int H, int W, int t0, int nt) {
    const int WW = fh_words(W), S = fh_stride(W);
    const int last_bit = (W - 1) & 31;
    bool changed = false;
    for (int y = t0; y < H; y += nt) {
        const uint32_t* f = fr + (size_t)y * S;
        uint32_t* r = re + (size_t)y * S;
        uint32_t carry = 1u;                                      // the pixel left of column 0 is outside the image: reached
        for (int c = 0; c < WW; ++c) {
            const uint32_t old = r[c], g = fh_fill_up(old, f[c], carry);
            if (g != old) { r[c] = g; changed = true; }
            carry = g >> 31;
        }
        carry = 1u;                                               // ... and so is the pixel right of column W - 1
        for (int c = WW - 1; c >= 0; --c) {
            const uint32_t old = r[c];
            uint32_t g;
            if (c == WW - 1 && last_bit != 31) {                  // the row ends inside this word: the carry enters at its last pixel
                g = old | (f[c] & (1u << last_bit));
                g = fh_fill_down(g, f[c], 0u);
            } else {
                g = fh_fill_down(old, f[c], carry);
            }
            if (g != old) { r[c] = g; changed = true; }
            carry = g & 1u;
        }
    }
    return changed;
}

// word columns t0, t0 + nt, ...: both vertical sweeps
__host__ __device__ inline bool fh_sweep_cols(const uint32_t* fr, uint32_t* re, int H, int W, int t0, int nt) {
    const int WW = fh_words(W), S = fh_stride(W);
    bool changed = false;
    for (int c = t0; c < WW; c += nt) {
        uint32_t prev = 0xffffffffu;                              // the row above row 0 is outside the image
        for (int y = 0; y < H; ++y) {
            const size_t i = (size_t)y * S + c;
            const uint32_t old = re[i], g = old | (prev & fr[i]);
            if (g != old) { re[i] = g; changed = true; }
            prev = g;
        }
        prev = 0xffffffffu;
        for (int y = H - 1; y >= 0; --y) {
            const size_t i = (size_t)y * S + c;
            const uint32_t old = re[i], g = old | (prev & fr[i]);
            if (g != old) { re[i] = g; changed = true; }
            prev = g;
        }
    }
    return changed;
}

// The pass loop on planes that hold `free` and a zeroed `reached`.  vote: two words (zeroed), shared by the workgroup.  Every thread returns
// the same value: true = stable, false = the bound was reached.
template <typename Sync>
__host__ __device__ inline bool fh_fill(const uint32_t* fr, uint32_t* re, int* vote, int H, int W, int t0, int nt, Sync sync) {
    const int bound = H * W + 1;
    for (int pass = 0; pass < bound; ++pass) {
        bool changed = fh_sweep_rows(fr, re, H, W, t0, nt);
        sync();
        if (t0 == 0) vote[(pass + 1) & 1] = 0;                    // the other word: last read behind the previous pass' barrier, next written behind the next
        changed = fh_sweep_cols(fr, re, H, W, t0, nt) || changed;
        if (changed) vote[pass & 1] = 1;
        sync();
        if (!vote[pass & 1]) return true;
    }
    return false;
}

struct FillP {
    int H, W;
    const float* x; float* out_f; uint8_t* out_u8; int32_t* error;
};

// grid (N), FH_THREADS threads; dynamic LDS: free plane | reached plane
__global__ __launch_bounds__(FH_THREADS) void fill_holes_kernel(const FillP p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t fh_lds[];
    __shared__ int vote[2];
    const int H = p.H, W = p.W, WW = fh_words(W), S = fh_stride(W), tid = threadIdx.x;
    const size_t plane = fh_plane_words(H, W), img = blockIdx.x;
    uint32_t* fr = fh_lds;
    uint32_t* re = fh_lds + plane;
    const float* x = p.x + img * (size_t)H * W;
    for (int i = tid; i < (int)plane; i += FH_THREADS) { fr[i] = 0u; re[i] = 0u; }      // the pad word of every row included
    if (tid < 2) vote[tid] = 0;
    __syncthreads();
    // 64 consecutive pixels of a row per wave step: one coalesced load, one ballot, two plane words
    const int lane = tid & 63, wave = tid >> 6, chunks = (W + 63) >> 6;
    for (int j = wave; j < H * chunks; j += FH_THREADS / 64) {
        const int y = j / chunks, c64 = j - y * chunks, xx = c64 * 64 + lane;
        const bool in = xx < W;
        const float v = in ? x[(size_t)y * W + xx] : 0.f;
        const unsigned long long fg = __ballot(in && sigmoidf_(v) > 0.5f), inside = __ballot(in);
        const unsigned long long fre = ~fg & inside;
        if (lane == 0) {
            fr[(size_t)y * S + 2 * c64] = (uint32_t)fre;
            if (2 * c64 + 1 < WW) fr[(size_t)y * S + 2 * c64 + 1] = (uint32_t)(fre >> 32);
        }
    }
    __syncthreads();
    const bool stable = fh_fill(fr, re, vote, H, W, tid, FH_THREADS, DevSync());
    if (!stable && tid == 0) *p.error = 1;
    // filled = not reached; four pixels per thread step (W % 16 == 0: they share a row and a word)
    const int quads = H * W / 4;
    for (int q = tid; q < quads; q += FH_THREADS) {
        const int pix = q * 4, y = pix / W, xx = pix - y * W;
        const uint32_t bits = (re[(size_t)y * S + (xx >> 5)] >> (xx & 31)) & 15u;
        const size_t o = img * (size_t)H * W + pix;
        if (p.out_f) {
            f32x4 v;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = ((bits >> k) & 1u) ? -1.f : 1.f;
            *reinterpret_cast<f32x4*>(p.out_f + o) = v;
        }
        if (p.out_u8) {
            uint32_t w = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) w |= ((bits >> k) & 1u) ? 0u : (255u << (8 * k));
            *reinterpret_cast<uint32_t*>(p.out_u8 + o) = w;
        }
    }
}

int fh_check(const mtbc_fill_holes_args* a) {
    if (!a) return MTBC_E_BADARG;
    if (a->N <= 0 || a->H < 16 || a->W < 16 || a->H > FH_MAX_DIM || a->W > FH_MAX_DIM || (a->H & 15) || (a->W & 15)) return MTBC_E_BADSHAPE;
    if (!a->seg_logits || !a->error || (!a->filled_logits && !a->filled_u8)) return MTBC_E_BADARG;
    return MTBC_OK;
}

}  // namespace

extern "C" int mtbc_fill_holes(const mtbc_fill_holes_args* a, void* stream) {
    const int rc = fh_check(a);
    if (rc != MTBC_OK) return rc;
    // the vector stores of the output pass: H * W % 16 == 0, so every image starts aligned when the base is
    if (((uintptr_t)a->seg_logits & 3) || (a->filled_logits && ((uintptr_t)a->filled_logits & 15)) || (a->filled_u8 && ((uintptr_t)a->filled_u8 & 3)))
        return MTBC_E_BADARG;
    FillP p;
    p.H = a->H; p.W = a->W; p.x = a->seg_logits; p.out_f = a->filled_logits; p.out_u8 = a->filled_u8; p.error = a->error;
    const size_t lds = 2 * fh_plane_words(a->H, a->W) * sizeof(uint32_t);
    MTBC_ENSURE_DYN_LDS(fill_holes_kernel, (int)(2 * fh_plane_words(FH_MAX_DIM, FH_MAX_DIM) * sizeof(uint32_t)));
    hipLaunchKernelGGL(fill_holes_kernel, dim3((unsigned)a->N), dim3(FH_THREADS), lds, (hipStream_t)stream, p);
    MTBC_CHECK_LAUNCH();
    return MTBC_OK;
}

extern "C" int mtbc_fill_holes_host(const mtbc_fill_holes_args* a) {
    const int rc = fh_check(a);
    if (rc != MTBC_OK) return rc;
    const int H = a->H, W = a->W, S = fh_stride(W);
    const size_t plane = fh_plane_words(H, W);
    uint32_t* fr = static_cast<uint32_t*>(calloc(2 * plane, sizeof(uint32_t)));
    if (!fr) return MTBC_E_WORKSPACE;
    uint32_t* re = fr + plane;
    for (int n = 0; n < a->N; ++n) {
        const float* x = a->seg_logits + (size_t)n * H * W;
        for (size_t i = 0; i < 2 * plane; ++i) fr[i] = 0u;
        for (int y = 0; y < H; ++y)
            for (int xx = 0; xx < W; ++xx)
                if (!(sigmoidf_(x[(size_t)y * W + xx]) > 0.5f)) fr[(size_t)y * S + (xx >> 5)] |= 1u << (xx & 31);
        int vote[2] = {0, 0};
        if (!fh_fill(fr, re, vote, H, W, 0, 1, HostSync())) *a->error = 1;
        for (int y = 0; y < H; ++y)
            for (int xx = 0; xx < W; ++xx) {
                const bool reached = (re[(size_t)y * S + (xx >> 5)] >> (xx & 31)) & 1u;
                const size_t o = ((size_t)n * H + y) * W + xx;
                if (a->filled_logits) a->filled_logits[o] = reached ? -1.f : 1.f;
                if (a->filled_u8) a->filled_u8[o] = reached ? 0 : 255;
            }
    }
    free(fr);
    return MTBC_OK;
}
