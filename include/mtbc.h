/*
 * mtbc.h -- C-ABI of libmtbc_hip.so: the MI355X (gfx950) hot path of the multi-task
 * conv encoder-decoder training step of caumente/multi_task_breast_cancer.
 *
 * The reference has no FFI of its own (it is pure Python on torch.nn); each
 * entry point below names the reference call it replaces (file:line, relative to the
 * upstream repository).  All tensors are fp32, NCHW, plane-contiguous (channel stride =
 * H*W) device pointers BORROWED from the caller until the stream operation completes; the
 * 16-bit compute modes may additionally hand the MFMA kernels their operand tensors -- and take
 * the conv outputs between a convolution and its norm -- in the matrix pipe's own format
 * (MTBC_LAYOUT_C8: bf16 / fp16, [N][C/8][H*W][8]) -- every such field says so where it is declared, and what the reference would see (parameters, gradients of
 * parameters, losses, logits) is fp32 in every mode.
 *
 * Conventions: return 0 (MTBC_OK) or a negative MTBC_E_* code; never throws, never
 * allocates, never synchronises the device; deterministic (no float atomics); thread-safe
 * for distinct streams (no mutable process-wide state).  `stream` is a hipStream_t passed as void*.
 */
#ifndef MTBC_H
#define MTBC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTBC_VERSION 203            /* 0.2.3: Adam's own struct and its three entry points removed -- Adam is mtbc_optim_args with kind = MTBC_OPT_ADAMW and weight_decay = 0 -- and MTBC_OP_ADAM became MTBC_OP_OPTIM; 0.2.2 (round 4): Adam's `dynamic` scalars appended; 0.2.1: mtbc_conv3x3_args.wgrad_sync appended; 0.2.0: the argument structs grew in round 2 (fields appended); a binding compiled against
                                       another version must refuse the library (mtbc_version()) -- layouts are not negotiated */
#define MTBC_MAX_SEGS 6
#define MTBC_STEM_MAX_CIN 5         /* the stem kernels of mtbc_conv3x3_*: ONE fp32 planar input segment of 1 .. 5 channels -- the image plus the four
                                       intensity channels of data.augmentation (experiment_init.py:97, n_augments) */

enum {
    MTBC_OK = 0,
    MTBC_E_BADSHAPE = -1,
    MTBC_E_BADARG = -2,
    MTBC_E_WORKSPACE = -3,
    MTBC_E_LAUNCH = -4,
    MTBC_E_UNSUPPORTED = -5
};

int mtbc_version(void);
const char* mtbc_strerror(int code);
/* name of the GPU architecture the device code was built for ("gfx950") */
const char* mtbc_arch(void);

/* A channel segment of a virtually concatenated NCHW tensor (replaces torch.cat(dim=1),
 * MTnnUNet.py:161-169,174; MTUNetPlusPlus.py:107-118,128).  Element (n, c, y, x) of the
 * segment lives at ptr[n*batch_stride + c*H*W + y*W + x].  `accumulate` is honoured when
 * the segment is an OUTPUT (gradient fan-in): 0 = overwrite, 1 = add to what is there;
 * 2 (mtbc_conv3x3_dgrad with operand_layout C8 only) = overwrite a 16-BIT planar (N,C,H,W)
 * segment of the type of `compute` (ptr 8-byte aligned, batch_stride in 16-bit elements): the
 * fp32 result rounded to nearest even -- for a gradient whose only reader rounds it to that
 * type anyway (the k = 2 transposed conv backward, mtbc_convT_args.dy_type16);
 * 3 (same call) = overwrite a 16-BIT CHANNEL-BLOCKED segment [N][channels/8][H*W][8] of that type (MTBC_LAYOUT_C8;
 * ptr 16-byte aligned, batch_stride in 16-bit elements, channels % 8 == 0) -- for a gradient with this one writer
 * whose reader takes the layout (mtbc_instnorm_args.dy_layout).  Either every segment of a launch has mode 3 or none. */
typedef struct {
    float* ptr;
    int64_t batch_stride;   /* elements */
    int32_t channels;
    int32_t accumulate;
} mtbc_seg;

/* ---------------------------------------------------------------- conv 3x3, stride 1, pad 1
 * replaces nn.Conv2d(k=3, padding=1): MTnnUNet.py:12-16 ; MONAI Convolution in
 * MTUNetPlusPlus.py:47-81.  Weight layout = torch (Cout, Cin, 3, 3).                       */
typedef struct {
    int32_t N, H, W, Cin, Cout;
    int32_t n_in;                    /* fwd/wgrad: input segments (sum channels == Cin)      */
    mtbc_seg in[MTBC_MAX_SEGS];      /* dgrad: OUTPUT dx segments (accumulate honoured)      */
    const float* w;                  /* (Cout,Cin,3,3)                                       */
    const float* w_packed;           /* fwd: mtbc_conv3x3_pack_fwd image, dgrad: _pack_dgrad;
                                        NULL selects the direct (non-MFMA) kernel           */
    const float* bias;               /* (Cout) or NULL                                       */
    float* out;                      /* fwd: z (N,Cout,H,W) ; dgrad: unused                  */
    const float* dout;               /* dgrad/wgrad: dz (N,Cout,H,W)                         */
    float* dw;                       /* wgrad: (Cout,Cin,3,3), overwritten or accumulated    */
    float* dbias;                    /* wgrad: (Cout) or NULL                                */
    int32_t accumulate_dw;           /* wgrad: 1 = add into dw/dbias (shared modules, F10)   */
    int32_t force_direct;            /* 1 = never use the MFMA kernels (debug / tests)       */
    void* workspace;                 /* wgrad split-K partials                               */
    size_t workspace_bytes;
    int32_t compute;                 /* MFMA operand type: 0 = fp32 (exact, the parity path), 1 = bf16,
                                        2 = fp16 -- storage and accumulation stay fp32; fwd/dgrad then need
                                        w_packed from mtbc_conv3x3_pack_lp                    */
    int32_t operand_layout;          /* how the tensors the MFMA READS are stored (fwd: `in`; dgrad: `dout`;
                                        wgrad: `in` and `dout`):
                                          0 = fp32 planar (N,C,H,W), converted while staging (default);
                                          1 = MTBC_LAYOUT_C8: already in the 16-bit type of `compute` (1 or 2),
                                              channel-blocked [N][C/8][H*W][8] (mtbc_c8_pack) -- pointers are
                                              passed through the float* / const float* fields, batch strides count
                                              16-bit elements, every segment holds a multiple of 8 channels and is
                                              16-byte aligned.  What the kernels WRITE (z, dx segments, dw, dbias)
                                              stays fp32 planar unless out_layout / a segment mode says otherwise.  No fallback: shapes the MFMA kernels do not take
                                              (W % 4 != 0, H or W < 8) return MTBC_E_UNSUPPORTED.                 */
    int32_t out_accumulate;          /* fwd with operand_layout C8 only: 1 = add the result to `out` instead of overwriting
                                        it.  A forward launch over the dz of ALL 3x3 consumers of a tensor, with
                                        mtbc_conv3x3_weight_view(mode 1) weights, is that tensor's gathered dgrad.  */
    int32_t out_layout;              /* fwd with operand_layout C8 -- or the stem: operand_layout 0, n_in = 1, Cin <= MTBC_STEM_MAX_CIN, W % 4 == 0,
                                        16-byte aligned, batch_stride % 4 == 0, compute 1 | 2, exact fp32 arithmetic; with planar operands anything
                                        else (Cin > MTBC_STEM_MAX_CIN, n_in > 1) is MTBC_E_UNSUPPORTED; the stem's weight gradient takes its dz in
                                        MTBC_LAYOUT_C8 with the same fp32 planar segment in `in` -- : MTBC_LAYOUT_C8 = `out` is written as a 16-bit
                                        channel-blocked tensor [N][Cout/8][H*W][8] of the type of `compute` (fp32 accumulate,
                                        + bias, ONE round-to-nearest-even) instead of fp32 planes: the conv output of the
                                        16-bit modes, read by mtbc_instnorm_args.z_layout = C8 (what torch.autocast stores
                                        between a convolution and its normalisation).  Cout % 8 == 0, out 16-byte aligned,
                                        out_accumulate = 0.                                                             */
    float* stats_partial;            /* fwd with out_layout C8 only, or NULL: InstanceNorm statistics from the conv EPILOGUE
                                        (MTnnUNet.py:30-38, MONAI ADN in MTUNetPlusPlus.py:20-22: the norm that follows every
                                        3x3 conv).  [N][slots][Cout][2] floats, slots = mtbc_conv3x3_stats_slots(args): per
                                        image, per wave-sized pixel subset and per channel {sum, sum of squares} of the STORED
                                        (rounded) outputs, fp32, no atomics; mtbc_instnorm_lrelu_fwd(stats_partial, stats_slots)
                                        combines them (fixed order, in double) and the normalisation becomes one streaming
                                        pass with no reduction of its own.                                                  */
    /* A gathered dgrad (forward-type launch over the dz of a tensor's 3x3 consumers, out_layout C8) can also prepare the
       InstanceNorm + LeakyReLU BACKWARD of the tensor it differentiates (all optional, norm_z selects it):
         out_partial : fp32 planar (N,Cout,H,W) partial gradient written by the tensor's other readers (pool / ConvT / 1x1
                       backward), added in fp32 BEFORE the one rounding of `out`;
         norm_z      : the tensor's own conv output z, 16-bit channel-blocked like `out`; norm_mean / norm_rstd (N*Cout),
                       norm_gamma / norm_beta (Cout or NULL), norm_slope: its InstanceNorm + LeakyReLU;
       stats_partial then receives, per image, pixel subset and channel, {sum g, sum g * xhat} with g = dy * lrelu'(.) of the
       STORED dy -- the two reductions of the norm's backward (mtbc_instnorm_lrelu_bwd(stats_partial, stats_slots) becomes
       one streaming pass).                                                                                               */
    const float* out_partial;
    const void* norm_z;
    const float* norm_mean;
    const float* norm_rstd;
    const float* norm_gamma;
    const float* norm_beta;
    float norm_slope;
    int32_t out_type;                /* fwd with out_layout C8: 0 = the type of `compute`; 2 with compute = 1 (bf16 operands): the
                                        output is stored as fp16 (saturated at +-65504) -- for conv outputs of O(1) that a norm
                                        follows: 11 significant bits in the same 2 bytes (mtbc_instnorm_args.z_type)              */
    int32_t* wgrad_sync;             /* wgrad with operand_layout C8 (Cin >= 8), or NULL: mtbc_conv3x3_wgrad_sync_bytes(args) bytes of
                                        ZEROED device memory (4-byte aligned) that stay the caller's between launches.  With it the
                                        split-K partials are reduced INSIDE the weight-gradient launch -- the block that stores the last
                                        partial of a group sums the group in row order (deterministic; no block waits for another, no
                                        co-residency requirement), a tree of 1 - 3 levels whose top writes dw / dbias -- instead of by a
                                        second launch.  Every counter is back at zero when the launch ends: one buffer serves all the
                                        launches of a stream, in order.  Launches on DIFFERENT streams need different buffers.  (backward
                                        of nn.Conv2d in MTUNetPlusPlus.py:47-81 / MTnnUNet.py:12-16, training_multitask.py:102)       */
    size_t wgrad_sync_bytes;
} mtbc_conv3x3_args;
#define MTBC_LAYOUT_PLANAR 0
#define MTBC_LAYOUT_C8 1

/* Views of a (Cout,Cin,3,3) weight for backward launches that cover only part of a conv's input channels:
 *   mode 0: dst (Cout, ci_cnt, 3, 3)  = w[:, ci_off : ci_off + ci_cnt]                 -- dgrad into a suffix of the segments
 *   mode 1: dst (ci_cnt, K, 3, 3)[:, k_off : k_off + Cout] = that slice transposed with flipped taps, i.e. the weight of
 *           the FORWARD conv over dz that computes the slice's input gradient; several convs fill one dst side by side
 *           (K = sum of their Cout): one launch then produces the gradient of a tensor from all its consumers
 *           (no read-modify-write fan-in).  Rebuilt every step like the packed images.                              */
int mtbc_conv3x3_weight_view(const float* w, float* dst, int32_t Cout, int32_t Cin, int32_t ci_off, int32_t ci_cnt, int32_t mode,
                             int32_t k_off, int32_t K, void* stream);
/* Batched form: every weight view a step needs in one launch (they are rebuilt after each optimizer update). */
typedef struct mtbc_wview_desc {
    const float* w;
    float* dst;
    int32_t Cout, Cin, ci_off, ci_cnt, mode, k_off, K;
} mtbc_wview_desc;
int mtbc_conv3x3_weight_view_many(const mtbc_wview_desc* descs, int32_t n, void* stream);

/* fp32 planar (N,C,H,W; batch stride in elements) -> 16-bit channel-blocked [N][C/8][H*W][8] in the type of
 * `compute` (1 = bf16, 2 = fp16; round to nearest even -- the same conversion the staging of operand_layout 0 does),
 * and back (exact).  C % 8 == 0, dst 16-byte aligned.  Producers that write this layout themselves (next step:
 * InstanceNorm+LeakyReLU, pooling, ConvTranspose) make the 3x3 convolutions' staging pure LDS-DMA.           */
int mtbc_c8_pack(const float* src, int64_t src_batch_stride, void* dst, int32_t N, int32_t C, int32_t HW, int32_t compute, void* stream);
int mtbc_c8_unpack(const void* src, float* dst, int32_t N, int32_t C, int32_t HW, int32_t compute, void* stream);
/* 16-bit planar (N,C,H,W; batch stride in 16-bit elements) -> the same values channel-blocked [N][C/8][H*W][8].
 * Type-agnostic (moves 16-bit words).  C % 8 == 0, HW % 4 == 0, src 8-byte and dst 16-byte aligned.             */
int mtbc_c8_pack16(const void* src, int64_t src_batch_stride, void* dst, int32_t N, int32_t C, int32_t HW, void* stream);

size_t mtbc_conv3x3_packed_elems(int32_t Cin, int32_t Cout);          /* fwd image size      */
size_t mtbc_conv3x3_packed_dgrad_elems(int32_t Cin, int32_t Cout);    /* dgrad image size    */
int mtbc_conv3x3_pack_fwd(const float* w, float* packed, int32_t Cin, int32_t Cout, void* stream);
int mtbc_conv3x3_pack_dgrad(const float* w, float* packed, int32_t Cin, int32_t Cout, void* stream);
/* 16-bit operand images for compute = 1 (bf16) / 2 (fp16): [mtile][chunk32][tap][16][32] 16-bit elements;
 * dgrad = 0 packs the forward image, 1 the flipped/transposed dgrad image.  Pass as w_packed. */
size_t mtbc_conv3x3_packed_lp_elems(int32_t Cin, int32_t Cout, int32_t dgrad);
int mtbc_conv3x3_pack_lp(const float* w, void* packed, int32_t Cin, int32_t Cout, int32_t dgrad, int32_t compute, void* stream);

/* Batched form of the four pack entry points above: every weight image a step needs in one launch (the images are
 * re-made after each optimizer update; ~70 tiny launches cost more than the copies).  kind: 0 = mtbc_conv3x3_pack_fwd,
 * 1 = _pack_dgrad, 2 = _pack_lp(dgrad=0), 3 = _pack_lp(dgrad=1); `compute` (1 bf16 | 2 fp16) is read for kinds 2,3. */
typedef struct mtbc_pack_desc {
    const float* w;
    void* packed;
    int32_t Cin, Cout;
    int32_t kind, compute;
} mtbc_pack_desc;
int mtbc_conv3x3_pack_many(const mtbc_pack_desc* descs, int32_t n, void* stream);
/* pixel subsets per image of the forward launch these arguments select (0: the launch does not produce statistics) */
int32_t mtbc_conv3x3_stats_slots(const mtbc_conv3x3_args* a);
size_t mtbc_conv3x3_wgrad_workspace(const mtbc_conv3x3_args* a);
/* bytes of zeroed counters mtbc_conv3x3_args.wgrad_sync needs for these arguments (0: this launch has no in-kernel reduction) */
size_t mtbc_conv3x3_wgrad_sync_bytes(const mtbc_conv3x3_args* a);
/* Host-only plan query: the kernel instance mtbc_conv3x3_fwd / _dgrad / _wgrad (op = MTBC_OP_CONV3_FWD / _DGRAD / _WGRAD) would
 * launch for these arguments, written to buf (NUL-terminated) as a profiler spells it without namespace and argument list, e.g.
 * "conv3x3_igemm_c8_kernel<3, 0, false, 4, 3>"; for the weight gradient followed by its reduction: " + splitk_reduce" (a reduction
 * launch), " + splitk_fixup" (in the kernel, mtbc_conv3x3_args.wgrad_sync), " + channel_sums" (the bias gradient's launch).
 * Launches nothing, never synchronises, never dereferences a tensor pointer; returns the code the real call would return when it
 * refuses the arguments, MTBC_E_BADARG for an unknown op or a buffer shorter than the name. */
int mtbc_conv3x3_kernel_name(const mtbc_conv3x3_args* a, int32_t op, char* buf, int32_t len);
/* Host-only plan query of the weight gradient: the numbers mtbc_conv3x3_wgrad hands the kernel that mtbc_conv3x3_kernel_name names -- how
 * the kernel walks its pixels is decided from N and the map size, which the name does not carry.  Filled on the path that launches (the
 * same dispatcher called without a stream).  A field the family does not read is 0.
 *   tile-walking kernels (conv3x3_wgrad_c8_kernel, _mfma_, _lp_, _lp2_): nsplit blocks walk total_tiles = tiles_x * tiles_y * images
 *     (geo 2: one tile = two images); split s owns tiles [s * tiles_per_split, ...) -- or, tiles_per_split < 0: dealt evenly,
 *     [s * total_tiles / nsplit, (s + 1) * total_tiles / nsplit);
 *   conv3x3_wgrad_c8w_kernel: tiles_x strips per image x segs row segments of seg_tiles 4-row steps (tiles_y steps per strip), a ring
 *     of 6 + 4 * depth rows; coblocks x ciblocks channel blocks of cit 16-channel input tiles;
 *   conv3x3_wgrad_c8i_kernel: segs image ranges of seg_tiles images; coblocks, ciblocks, cit as above;
 *   stem / small-Cin kernels: bands row bands per image (nsplit = N * bands);
 *   direct kernel: split s takes images s, s + nsplit, ...: images_per_split = the most one split takes.
 * reduce: what sums the nsplit partial rows -- MTBC_WGRAD_REDUCE_NONE (one split stores into dw), _LAUNCH (reduce_kernel = the
 * splitk_reduce instance, "splitk_reduce<16>"), _FIXUP (inside the kernel: a tree of fix_levels levels of fan-in fix_fanin). */
typedef struct {
    int32_t nsplit, total_tiles, tiles_per_split, tiles_x, tiles_y;
    int32_t coblocks, ciblocks, cit, segs, seg_tiles, depth;
    int32_t geo;
    int32_t bands;
    int32_t images_per_split;
    int32_t reduce;
    int32_t fix_levels, fix_fanin;
    char reduce_kernel[28];
} mtbc_wgrad_plan;
#define MTBC_WGRAD_REDUCE_NONE 0
#define MTBC_WGRAD_REDUCE_LAUNCH 1
#define MTBC_WGRAD_REDUCE_FIXUP 2
/* Launches nothing, never dereferences a tensor pointer; returns what mtbc_conv3x3_wgrad would return when it refuses the arguments
 * (a short workspace included), MTBC_E_BADARG for plan = NULL. */
int mtbc_conv3x3_wgrad_plan(const mtbc_conv3x3_args* a, mtbc_wgrad_plan* plan);
int mtbc_conv3x3_fwd(const mtbc_conv3x3_args* a, void* stream);
int mtbc_conv3x3_dgrad(const mtbc_conv3x3_args* a, void* stream);
int mtbc_conv3x3_wgrad(const mtbc_conv3x3_args* a, void* stream);

/* ------------------------------------------------- InstanceNorm2d(eps, affine?) + LeakyReLU
 * replaces nn.InstanceNorm2d + nn.LeakyReLU: MTnnUNet.py:35-36 (no affine, slope 0.01);
 * MONAI ADN "NDA" in MTUNetPlusPlus.py:20-22 (affine, slope 0.1).
 *   y = lrelu(gamma * (z - mean) * rstd + beta), biased variance over H*W per (n, c).
 * The output may be a channel slice of a wider buffer (out_batch_stride).                   */
typedef struct {
    int32_t N, C, H, W;
    float eps, slope;
    const float* z;          /* (N,C,H,W) conv output                                        */
    const float* gamma;      /* (C) or NULL                                                  */
    const float* beta;       /* (C) or NULL                                                  */
    float* y;                /* activation, element (n,c,p) at y[n*y_batch_stride + c*HW + p] */
    int64_t y_batch_stride;
    float* mean;             /* (N*C) saved for backward                                     */
    float* rstd;             /* (N*C)                                                        */
    /* backward */
    const float* dy;         /* grad wrt y, same addressing as y (dy_batch_stride)           */
    int64_t dy_batch_stride;
    int32_t n_dy_extra;      /* gradient fan-in: up to 4 more contributions, added to dy on the */
    const float* dy_extra[4];/* fly (same addressing) -- each consumer of y writes its own buffer
                                with plain stores instead of read-modify-write accumulation      */
    float* dz;               /* (N,C,H,W) grad wrt z                                         */
    float* dgamma;           /* (C) or NULL */
    float* dbeta;            /* (C) or NULL */
    float* dbias_pre;        /* (C) or NULL: gradient of a per-channel bias added in front of the
                                norm (the conv bias) = sum over n,h,w of dz, fused here so the
                                conv wgrad does not re-read dz                                 */
    int32_t accumulate_dparams;
    void* workspace;         /* bwd with any of the three: N*C*3 floats (N*C*131 with dz8)    */
    size_t workspace_bytes;
    /* 16-bit planar outputs (the 16-bit compute modes): when y16 / dz16 is set, the forward activation / the
       backward dz is written ONLY as a 16-bit (N,C,H,W) tensor of type out16_type (1 = bf16, 2 = fp16; round to
       nearest even of the fp32 value) and y / dz is not touched -- for tensors that nothing but the 3x3 convs' MFMAs
       read (mtbc_c8_pack16 then brings them into MTBC_LAYOUT_C8): 2 instead of 4 bytes written and re-read.
       Register-resident planes only (H*W % 4 == 0, H*W <= 65536), else MTBC_E_UNSUPPORTED.            */
    void* y16;
    void* dz16;
    int32_t out16_type;
    /* 16-bit CHANNEL-BLOCKED outputs (MTBC_LAYOUT_C8, [N][C/8][H*W][8] of type out16_type): the forward activation
       goes to y8 (and, if y != NULL, also to y as fp32 planes), the backward dz to dz8 only.  One HBM pass by a
       cooperative kernel (csrc/norm_coop.hip: teams of resident workgroups exchange per-channel partials through
       coop_state).  coop_state: mtbc_instnorm_coop_state_bytes() of device memory, ZEROED once by the caller, kept
       for the lifetime of the stream's launches and never used from two streams at once.  C % 8 == 0, no dy_extra;
       shapes: ask mtbc_instnorm_c8_supported.  Statistics are combined with Chan's formula (fixed order).
       y8 together with y16 (forward with stats_partial only, H*W % 8 == 0; otherwise MTBC_E_UNSUPPORTED): the PLANAR copy is
       the 16-bit one -- the same rounded values as y8, for a reader that wants planes of the MFMA type
       (mtbc_convT_args.x_type16) -- and y is not touched; y_batch_stride then counts 16-bit elements of y16 (% 8 == 0).  */
    void* y8;
    void* dz8;
    void* coop_state;
    /* CUs this launch leaves out of the cooperative grid (0 = none): the teams need every member resident at once, and
       kernels of OTHER streams that hold CUs while it runs (RCCL collectives overlapping the backward pass) would make
       members wait for a slot.  Per call -- the library keeps no process-wide setting.                              */
    int32_t coop_reserve_cus;
    /* 16-bit channel-blocked INPUTS (with y8 / dz8 outputs only; type out16_type, C % 8 == 0, 16-byte aligned):
       z_layout  = MTBC_LAYOUT_C8: z is [N][C/8][H*W][8] as written by mtbc_conv3x3_fwd(out_layout = C8); statistics are
                   those of the stored (rounded) values, accumulated in fp32;
       dy_layout = MTBC_LAYOUT_C8: dy is [N][C/8][H*W][8] as written by mtbc_conv3x3_dgrad (segment mode 3) or by a
                   gathered forward-type launch with out_layout = C8 (dy_batch_stride in 16-bit elements); with
                   n_dy_extra = 1, dy_extra[0] is an fp32 planar (N,C,H,W) partial gradient from the tensor's other
                   readers (batch stride C*H*W), added to it in fp32 while loading.                                     */
    int32_t z_layout;
    int32_t dy_layout;
    /* forward with z_layout C8 and y8: the statistics come from the producing convolution's epilogue
       (mtbc_conv3x3_args.stats_partial, [N][stats_slots][C][2]); mean / rstd are still written for the backward pass.
       backward with z_layout C8, dy_layout C8 and dz8: {sum g, sum g * xhat} come from the gathered dgrad that wrote dy
       (mtbc_conv3x3_args.norm_z); the conv-bias gradient dbias_pre (mathematically zero in front of a norm) is then written
       as exact zeros instead of the rounding noise of a sum.  workspace: N*C*5 floats.                                  */
    const float* stats_partial;
    int32_t stats_slots;
    int32_t z_type;                  /* with z_layout C8: 0 = z has the type of out16_type; 2 = z is fp16 although out16_type is bf16 */
    /* backward with dz8: the input gradient of a ONE-output 1x1 conv head that reads this activation (MTUNetPlusPlus.py:73-76,
       final_conv_0_j) is rank 1 -- dy[n,c,p] += dy_rank1_w[c] * dy_rank1[n*H*W + p] -- and is formed here from the head's own
       gradient (N,1,H,W) and weight (C) instead of being written by mtbc_conv1x1_dgrad and read back; dy may then be NULL
       (a tensor nothing else reads).  Both NULL or both set.                                                                */
    const float* dy_rank1;
    const float* dy_rank1_w;
    /* ... and, optionally, that head's OWN parameter gradients (what mtbc_conv1x1_wgrad computes from the stored activation):
       dy_rank1_dw[c] (+)= sum_{n,p} y_stored[n,c,p] * dy_rank1[n,p] with y re-formed from z and rounded to out16_type,
       dy_rank1_db[0] (+)= sum dy_rank1.  workspace: N*C*(3 + 2T) + N*T floats, T = team size (131 -> 260 per plane covers it). */
    float* dy_rank1_dw;
    float* dy_rank1_db;
    int32_t dy_rank1_accumulate;
    /* backward with dz8: the gradient coming back through a MaxPool2d(2,2) that reads this activation (MTnnUNet.py:103, MONAI Down):
       dy[n,c,y,x] += dy_pool[n,c,y/2,x/2] if the window's maximum sits at (y,x) according to dy_pool_arg (mtbc_maxpool_args.argmax),
       formed while loading.  dy_pool: fp32 planar (N,C,H/2,W/2).  Both NULL or both set; H and W even.                          */
    const float* dy_pool;
    const void* dy_pool_arg;
    /* forward with stats_partial (the streaming pass): also write the activation's MaxPool2d(2,2) -- pool_y8: channel-blocked 16-bit
       [N][C/8][H/2*W/2][8] of out16_type, the maxima of the STORED values (= mtbc_maxpool2_fwd on y8, bit for bit, NaN and -0 / +0 windows included: both take the scan stated at mtbc_maxpool_args); pool_arg: optional
       argmax codes (mtbc_maxpool_args.argmax).  H and W even.                                                                     */
    void* pool_y8;
    void* pool_arg;
    int32_t defer_dparams;           /* backward with dz8 and any of dgamma / dbeta / dbias_pre: 1 = stop after the norm kernel: the
                                        per-plane partial sums stay in `workspace` (a buffer of the caller's that lives until
                                        mtbc_instnorm_dparam_many has reduced it) and dgamma / dbeta / dbias_pre are not touched --
                                        one launch for the parameter gradients of many cells instead of one 5 us launch each      */
} mtbc_instnorm_args;
size_t mtbc_instnorm_coop_state_bytes(void);
/* Byte offset, inside a coop_state block, of the 32-bit STICKY error word: non-zero once any cooperative launch on that
 * state gave up a bounded mailbox poll (a team member was not resident).  Every output of that launch and of the ones after
 * it is then garbage: callers read the word when they read their losses and stop (trainer.FusedTrainStep.check_nan).   */
size_t mtbc_instnorm_coop_error_offset(void);
int mtbc_instnorm_c8_supported(const mtbc_instnorm_args* a, int32_t backward);
/* team size of the channel-group backward these arguments select (1 for planes <= 64 x 64; 0: not supported) */
int32_t mtbc_instnorm_bwd_team(const mtbc_instnorm_args* a);
/* dgamma[c] (+)= sum_n part[n,c,1] ; dbeta[c] (+)= sum_n part[n,c,0] ; dbias_pre[c] (+)= sum_n (part[n,c,2] + sum_m part3[n,c,m]) for
 * every descriptor in ONE launch, from the partials a deferred backward left: part = workspace, part3 = workspace + 3*N*C (T floats per
 * plane).  Same summation order as the reduction inside mtbc_instnorm_lrelu_bwd.                                                   */
typedef struct mtbc_dparam_desc {
    const float* part;
    float* dgamma;                   /* (C) or NULL */
    float* dbeta;                    /* (C) or NULL */
    float* dbias_pre;                /* (C) or NULL */
    int32_t N, C, T, accumulate;
} mtbc_dparam_desc;
int mtbc_instnorm_dparam_many(const mtbc_dparam_desc* descs, int32_t n, void* stream);

/* workspace bytes the forward can use for planes > 64K elements (chunked statistics: 2 reads + 1 write instead of the
 * streaming kernel's 3 + 1); 0 for smaller planes.  Passing no workspace is valid (streaming kernel). */
size_t mtbc_instnorm_fwd_workspace(const mtbc_instnorm_args* a);
/* Plan query: every launch mtbc_instnorm_lrelu_fwd (backward = 0) / mtbc_instnorm_lrelu_bwd (backward != 0) would make for these
 * arguments, in order and joined with " + ", written to buf (NUL-terminated).  Each kernel is spelled as a profiler spells the instance,
 * without namespace and argument list; where the dispatcher and not the template chooses the block size, " [threads=256]" follows; a
 * cooperative (team) launch carries its plan, e.g. "in_bwd_c8_kernel<512, 4, false, true, 2, 0> [T=32 rounds=4] + in_r1_finalize_kernel +
 * in_dparam_kernel" (T workgroups per team, rounds = items per resident team).  The follow-up launches are named too: in_stats_finalize_kernel,
 * in_bstats_finalize_kernel, in_r1_finalize_kernel, in_dparam_kernel (absent with defer_dparams: mtbc_instnorm_dparam_many reduces later).
 * It is the dispatcher of the real call, stopped in front of its launches: launches nothing, never synchronises, never dereferences a
 * tensor pointer (pointer VALUES are looked at: NULL selects branches, alignment the vector kernels); returns the code the real call
 * would return when it refuses the arguments, MTBC_E_BADARG for a buffer shorter than the name.  Device access: for planes above 64 x 64
 * with y8 / dz8 the team plan comes from the occupancy of the kernel on the current device and its CU count, asked once per device as the
 * launch asks them; without a GPU that plan does not exist and the query returns what the launch would, MTBC_E_UNSUPPORTED.  Everything
 * else is host arithmetic. */
int mtbc_instnorm_kernel_name(const mtbc_instnorm_args* a, int32_t backward, char* buf, int32_t len);
int mtbc_instnorm_lrelu_fwd(const mtbc_instnorm_args* a, void* stream);
int mtbc_instnorm_lrelu_bwd(const mtbc_instnorm_args* a, void* stream);

/* --------------------------------------------------------------------- MaxPool2d(2, 2)
 * replaces nn.MaxPool2d(2,2): MTnnUNet.py:103 ; MONAI Down in MTUNetPlusPlus.py:48-51.
 * ONE definition of a window's maximum for the forward value, the argmax codes, the backward routing and the pool the streaming
 * InstanceNorm pass writes (mtbc_instnorm_args.pool_y8) -- ATen's scan: in (0,0),(0,1),(1,0),(1,1) order an element replaces the running
 * maximum when it is greater or a NaN.  So: the FIRST of equal maxima (-0 and +0 are equal: a window {-0, +0, ..} pools to -0), and a NaN
 * is the maximum wherever it sits (the last of several).  fwd stores that element; bwd routes dy to it.  */
typedef struct {
    int32_t N, C, H, W;              /* INPUT spatial size; output is H/2 x W/2              */
    const float* x;  int64_t x_batch_stride;
    float* y;        int64_t y_batch_stride;
    const float* dy; int64_t dy_batch_stride;
    float* dx;       int64_t dx_batch_stride;
    int32_t accumulate_dx;
    int32_t layout;                  /* 0 = fp32 planar x / y.  MTBC_LAYOUT_C8 (the 16-bit compute modes): x and y are 16-bit
                                        channel-blocked [N][C/8][H*W][8] of type16 (1 = bf16, 2 = fp16), batch strides in
                                        16-bit elements, C % 8 == 0 -- forward = the fp32 pool of the stored values followed
                                        by mtbc_c8_pack, bit for bit (selecting a stored value commutes with rounding); backward routes on the
                                        stored values; dy / dx stay fp32 planar                                            */
    int32_t type16;
    void* argmax;                    /* fwd with layout C8, optional: (N, C/8, H/2 * W/2) 16-bit codes, bits [2c+1 : 2c] = which of the four
                                        window positions (0,0),(0,1),(1,0),(1,1) holds the first maximum of channel 8g + c -- where the
                                        backward routes the gradient.  With it the backward of the pool can be formed inside the
                                        InstanceNorm backward of the pooled tensor (mtbc_instnorm_args.dy_pool) instead of writing a
                                        4x larger, three-quarters-zero fp32 tensor that is read back                                   */
} mtbc_maxpool_args;

int mtbc_maxpool2_fwd(const mtbc_maxpool_args* a, void* stream);
int mtbc_maxpool2_bwd(const mtbc_maxpool_args* a, void* stream);

/* --------------------------------------------------------------------- Upsample(scale_factor=2, mode="nearest")
 * replaces nn.Upsample(scale_factor=2, mode="nearest"): Multi_BTS_UNet.py:100,154-158.
 *   fwd  y[n,c,2h+a,2w+b] = x[n,c,h,w] for a, b in {0,1}: a bit copy (NaN payloads and the sign of zero travel)
 *   bwd  dx[n,c,h,w] (+)= (dy[2h,2w] + dy[2h,2w+1]) + (dy[2h+1,2w] + dy[2h+1,2w+1]), in that order, in fp32
 * No workspace, no atomics: every element of y / dx is written by one thread of one launch.                       */
typedef struct {
    int32_t N, C, H, W;              /* INPUT spatial size; output is 2H x 2W                */
    const void* x;   int64_t x_batch_stride;
    void* y;         int64_t y_batch_stride;
    int32_t layout;                  /* fwd: 0 = fp32 planar x / y.  MTBC_LAYOUT_C8: x and y are 16-bit channel-blocked
                                        [N][C/8][H*W][8] / [N][C/8][4*H*W][8], batch strides in 16-bit elements (multiples of 8),
                                        C % 8 == 0, 16-byte aligned: a pixel's 8 channels move as one 16-byte word, so bf16 and fp16
                                        share one kernel                                                                   */
    int32_t type16;                  /* 1 = bf16, 2 = fp16 with layout C8 (recorded, not interpreted); 0 with fp32 planes   */
    const float* dy; int64_t dy_batch_stride;      /* bwd: fp32 planes (N,C,2H,2W) whatever `layout` says                   */
    float* dx;       int64_t dx_batch_stride;      /*      fp32 planes (N,C,H,W)                                            */
    int32_t accumulate_dx;           /* bwd: 0 = dx is overwritten, 1 = read-modify-written (the tensor has another reader) */
} mtbc_upsample2_args;
int mtbc_upsample2_fwd(const mtbc_upsample2_args* a, void* stream);
int mtbc_upsample2_bwd(const mtbc_upsample2_args* a, void* stream);

/* --------------------------------------------- ConvTranspose2d, kernel == stride == k
 * replaces nn.ConvTranspose2d(k, stride=k): MTnnUNet.py:96-100,106-116 (k = 2, 4, 8);
 * MONAI UpSample("deconv") in UpCat.  Weight layout = torch (Cin, Cout, k, k).
 *   y[n,co,k*i+a,k*j+b] = bias[co] + sum_ci x[n,ci,i,j] * W[ci,co,a,b]                      */
typedef struct {
    int32_t N, H, W, Cin, Cout, k;   /* INPUT spatial size H x W; output kH x kW             */
    const float* x;  int64_t x_batch_stride;
    const float* w;
    const float* bias;               /* (Cout) or NULL */
    float* y;        int64_t y_batch_stride;
    const float* dy; int64_t dy_batch_stride;
    float* dx;       int64_t dx_batch_stride;
    int32_t accumulate_dx;
    float* dw;       float* dbias;
    int32_t accumulate_dw;
    void* workspace; size_t workspace_bytes;
    int32_t compute;                 /* k == 2 backward only: 0 = fp32 MFMA (exact), 1 = bf16, 2 = fp16 operands */
    int32_t y_layout;                /* fwd: 0 = fp32 planar y; MTBC_LAYOUT_C8 = y is written as 16-bit channel-blocked
                                        [N][Cout/8][k*H*k*W][8] (what a 3x3 conv with operand_layout C8 reads; batch
                                        stride in 16-bit elements) -- same fp32 arithmetic, one RNE at the store, i.e.
                                        bit-identical to the planar forward followed by mtbc_c8_pack                */
    int32_t y_type;                  /* with y_layout C8: 1 = bf16, 2 = fp16                                        */
    int32_t x_layout;                /* fwd: MTBC_LAYOUT_C8 = x is ALSO 16-bit channel-blocked (type y_type, batch stride in
                                        16-bit elements; needs y_layout C8): the forward then runs on the 16-bit MFMA
                                        with rounded x and w (fp32 accumulate, bias, one RNE) -- k == 2, Cin % 8 == 0  */
    int32_t dy_type16;               /* dgrad / wgrad, k == 2 with compute = 1 | 2 only: non-zero (= compute) says dy is a 16-BIT
                                        planar (N,Cout,kH,kW) tensor of that type (batch stride in 16-bit elements), as
                                        written by mtbc_conv3x3_dgrad into a segment with accumulate = 2; the MFMAs read it
                                        as is (what they did to an fp32 dy while loading it), the bias gradient is the
                                        sum of the stored values.  Shapes the direct kernels do not take: MTBC_E_UNSUPPORTED */
    int32_t x_type16;                /* wgrad, with dy_type16 only: non-zero (= compute) says x is a 16-BIT planar (N,Cin,H,W) tensor of
                                        that type too (batch stride in 16-bit elements, % 8 == 0), as written by
                                        mtbc_instnorm_lrelu_fwd into y16 beside y8: 8 pixels of a channel are one 16-byte load that
                                        is the MFMA fragment -- the operands the fp32 x gave after rounding, bit for bit      */
} mtbc_convT_args;
/* 1 if mtbc_convT_fwd takes these arguments with y_layout = MTBC_LAYOUT_C8 (fp32 x: k == 2, Cin <= 64, Cout <= 48,
 * Cout % 8 == 0, H*W % 32 == 0; x_layout C8: k == 2, channel counts % 8 == 0, H*W % 32 == 0), else 0: the caller then
 * keeps the planar forward and converts with mtbc_c8_pack.                                                     */
int mtbc_convT_fwd_c8_supported(const mtbc_convT_args* a);

size_t mtbc_convT_wgrad_workspace(const mtbc_convT_args* a);
int mtbc_convT_fwd(const mtbc_convT_args* a, void* stream);
int mtbc_convT_dgrad(const mtbc_convT_args* a, void* stream);
int mtbc_convT_wgrad(const mtbc_convT_args* a, void* stream);
/* Host-only plan query: every launch mtbc_convT_fwd / _dgrad / _wgrad (op = MTBC_OP_CONVT_FWD / _DGRAD / _WGRAD) would make for these
 * arguments, written to buf (NUL-terminated) and joined with " + ".  Kernels are spelled as a profiler spells the instance without
 * namespace and argument list, e.g. "convT2_bwd_fused_kernel<1, 2, 3, true>"; the follow-up launches are "splitk_reduce" (once for dW,
 * once more for a bias gradient the kernel summed on the way) and "channel_sums" (the bias gradient's own pass).  The plan facts that
 * select code paths inside a split-K kernel without being template arguments follow its name in brackets: "[splits=1]" or "[splits>1]",
 * with "xcd " in front where a split's tasks are ordered onto one XCD ("[xcd splits>1]").  dgrad_next (op = MTBC_OP_CONVT_WGRAD only, else
 * ignored; may be NULL): the arguments of the MTBC_OP_CONVT_DGRAD right behind the weight gradient in a program -- the name is then what
 * mtbc_program_run makes of the pair, the fused kernel where it takes it and the two calls' launches otherwise.  Launches nothing, never
 * synchronises, needs no device and never dereferences a tensor pointer (pointer VALUES count: NULL and alignment select branches);
 * returns the code the real call would return when it refuses the arguments, MTBC_E_BADARG for an unknown op or a buffer shorter than
 * the name. */
int mtbc_convT_kernel_name(const mtbc_convT_args* a, int32_t op, const mtbc_convT_args* dgrad_next, char* buf, int32_t len);

/* -------------------------------------------------------------------------- conv 1x1 + bias
 * replaces nn.Conv2d(k=1): MTnnUNet.py:6-9,106-118 ; MTUNetPlusPlus.py:73-76 (Cout = regions) */
typedef struct {
    int32_t N, H, W, Cin, Cout;
    const float* x;  int64_t x_batch_stride;
    const float* w;                  /* (Cout,Cin,1,1) */
    const float* bias;
    float* y;                        /* (N,Cout,H,W) */
    const float* dy;
    float* dx;       int64_t dx_batch_stride;
    int32_t accumulate_dx;
    float* dw;       float* dbias;
    int32_t accumulate_dw;
    void* workspace; size_t workspace_bytes;
    int32_t x_layout;                /* 0 = fp32 planar x.  MTBC_LAYOUT_C8: x is 16-bit channel-blocked [N][Cin/8][H*W][8] of
                                        x_type (1 = bf16, 2 = fp16; batch stride in 16-bit elements; Cin % 8 == 0, Cout <= 8):
                                        forward and weight gradient read the stored (rounded) activation with fp32 weights,
                                        products and sums (forward = mtbc_conv1x1_fwd on the unpacked tensor, bit for bit);
                                        y, dy, dx, dw stay fp32.  Ask mtbc_conv1x1_wgrad_workspace with the same fields set */
    int32_t x_type;
} mtbc_conv1x1_args;

size_t mtbc_conv1x1_wgrad_workspace(const mtbc_conv1x1_args* a);
int mtbc_conv1x1_fwd(const mtbc_conv1x1_args* a, void* stream);
int mtbc_conv1x1_dgrad(const mtbc_conv1x1_args* a, void* stream);
int mtbc_conv1x1_wgrad(const mtbc_conv1x1_args* a, void* stream);

/* ----------------------------------------------- AdaptiveAvgPool2d(1) + Flatten
 * replaces MTnnUNet.py:126-127 ; MTUNetPlusPlus.py:81-82                                    */
typedef struct {
    int32_t N, C, H, W;
    const float* x;  float* y;       /* y: (N,C) */
    const float* dy; float* dx;      /* dx: (N,C,H,W) overwritten */
} mtbc_gap_args;
int mtbc_gap_fwd(const mtbc_gap_args* a, void* stream);
int mtbc_gap_bwd(const mtbc_gap_args* a, void* stream);

/* ----------------------------------------------------------- Linear (+ optional ReLU)
 * replaces nn.Linear/nn.ReLU: MTnnUNet.py:128-131 ; MTUNetPlusPlus.py:83-86.
 * y = relu?(x W^T + b), W: (Out, In).  bwd needs y when relu != 0.                          */
typedef struct {
    int32_t N, In, Out, relu;
    const float* x; const float* w; const float* bias; float* y;
    const float* dy; float* dx;      /* dx (N,In) overwritten; may be NULL */
    float* dw; float* dbias; int32_t accumulate_dw;
    void* workspace; size_t workspace_bytes;   /* bwd with relu: N*Out floats; the batch-shared kernels: mtbc_linear_workspace */
} mtbc_linear_args;
int mtbc_linear_fwd(const mtbc_linear_args* a, void* stream);
int mtbc_linear_bwd(const mtbc_linear_args* a, void* stream);
/* Wide inputs (a flattened feature map: Multi_BTS_UNet.py:110, In = 16384 * width / 8): from In >= MTBC_LINEAR_WIDE_MIN_IN, with In % 4 == 0
 * and 16-byte aligned x, w (forward) / w, dx (input gradient), the forward and the input gradient run on batch-shared kernels: a block owns a
 * slab of W and ALL N samples (eight at a time), so W is read from memory once per launch instead of once per sample.  Split partials (over In
 * forward, over Out for dx) go to the workspace and are summed in a fixed order by a second launch: deterministic, no atomics.  Selected by
 * shape and alignment alone; below the threshold the launches are the per-sample ones.  dW keeps linear_dw_kernel (it writes W once already).
 * mtbc_linear_workspace: the bytes the call needs (backward != 0: mtbc_linear_bwd) for a->N, In, Out, relu and dx -- host arithmetic; 0 = none.
 * mtbc_linear_wide_enable: process-wide A/B switch of the batch-shared kernels (1 = on, the default); returns the previous value.  Off,
 * every Linear call makes the per-sample launches and the workspace query answers for them.                                              */
#define MTBC_LINEAR_WIDE_MIN_IN 4096
size_t mtbc_linear_workspace(const mtbc_linear_args* a, int32_t backward);
int mtbc_linear_wide_enable(int32_t on);

/* ------------------------------------------------------------------------------ Dice loss
 * replaces monai.losses.DiceLoss(include_background=True, sigmoid=True, squared_pred=True,
 * smooth_nr=1, smooth_dr=1) built at experiment_init.py:210-211, fused over up to 4 deep
 * supervision heads with the 1/(j+1) weights of criterions.py:62.
 *   loss_h = mean_{n,c}( 1 - (2 I + nr) / (D + dr) ),  I = sum p t, D = sum p^2 + sum t^2
 * fwd : stats[h][n*C+c] = {I, P2, T2};  loss[h] = loss_h (unweighted);
 *       loss[n_heads] = sum_h head_weight[h] * loss_h
 * bwd : dx_h = gscale * head_weight[h] / (N*C) * d f / d x   (gscale: host scalar times an
 *       optional device scalar *gscale_dev, e.g. the upstream autograd gradient)
 *
 * `kind` selects the segmentation criterion (experiment_init.py:199-232, config key loss.function); the two calls, the head
 * weights, gscale, *gscale_dev and the layout of `loss` are the same for all of them.  p = sigmoid(x), HW = H * W, a plane = (n, c):
 *   MTBC_SEG_DICE (0)   the formula above.  A zero-initialised `kind` / `focal_gamma` is exactly the call as it was before they existed.
 *   MTBC_SEG_BCE        torch.nn.BCEWithLogitsLoss() (:225-226): loss_h = mean over N*C*HW of (1 - t) x + softplus(-x);
 *                       dx_h = gscale * head_weight[h] * (p - t) / (N*C*HW).  smooth_* unused.
 *   MTBC_SEG_FOCALDICE  MONAI 1.3.0 DiceFocalLoss(include_background, sigmoid, squared_pred, smooth_nr, smooth_dr) (:214-216):
 *                       the Dice formula above PLUS the mean over N*C*HW of m * bce, bce as for BCE, s = 2 t - 1,
 *                       m = exp(focal_gamma * logsigmoid(-x s)) (MONAI's sigmoid focal loss on the raw logits, gamma 2, no alpha,
 *                       lambda_dice = lambda_focal = 1).
 *   MTBC_SEG_JACCARD    MONAI DiceLoss(include_background, sigmoid, jaccard=True, reduction="sum") (:221-222; squared_pred=False,
 *                       smooth 1e-5 are MONAI's defaults -- the caller passes them in smooth_*): I = sum p t, P = sum p, T = sum t,
 *                       loss_h = SUM_{n,c}( 1 - (2 I + nr) / (2 (P + T - I) + dr) ); no 1/(N*C) in the loss or in dx_h.
 * (The two MONAI criteria are restated from knowledge of MONAI 1.3.0, as DiceLoss is: re-verify against a MONAI checkout.)
 * Statistics per (head, plane), MTBC_SEG_STATS_STRIDE(kind) floats each -- the caller sizes `stats` as n_heads * N*C * stride:
 *   DICE {I, sum p^2, sum t^2} (3) ; BCE {sum bce} (1) ; FOCALDICE {I, sum p^2, sum t^2, sum m bce} (4) ; JACCARD {I, P, T} (3)
 * MTBC_E_UNSUPPORTED: a kind outside the four.                                                                              */
#define MTBC_SEG_DICE 0
#define MTBC_SEG_BCE 1
#define MTBC_SEG_FOCALDICE 2
#define MTBC_SEG_JACCARD 3
#define MTBC_SEG_STATS_STRIDE(kind) ((kind) == MTBC_SEG_BCE ? 1 : (kind) == MTBC_SEG_FOCALDICE ? 4 : 3)
typedef struct {
    int32_t n_heads, N, C, H, W;
    float smooth_nr, smooth_dr;
    const float* x[4];               /* logits per head (N,C,H,W) */
    const float* target;             /* (N,C,H,W) */
    float head_weight[4];
    float* stats;                    /* n_heads * N*C * MTBC_SEG_STATS_STRIDE(kind) floats */
    float* loss;                     /* n_heads + 1 floats */
    float* dx[4];
    float gscale;
    const float* gscale_dev;         /* may be NULL */
    int32_t kind;                    /* MTBC_SEG_*; 0 = Dice */
    float focal_gamma;               /* MTBC_SEG_FOCALDICE only (the reference: 2) */
} mtbc_dice_args;
int mtbc_dice_fwd(const mtbc_dice_args* a, void* stream);
int mtbc_dice_bwd(const mtbc_dice_args* a, void* stream);

/* ----------------------------------------------------------------------------- Focal loss
 * replaces FocalLoss.forward (criterions.py:14-24, reduction='mean', soft/one-hot float
 * targets, optional class weight).  One launch computes the loss and d loss / d logits.
 *   ce_i = -sum_c w_c t_ic log_softmax(x_i)_c ; pt = exp(-ce_i) ;
 *   loss = mean_i alpha (1 - pt)^gamma ce_i ;  dx = gscale * (*gscale_dev) * d loss / d x
 * gamma = 0 is torch.nn.CrossEntropyLoss(reduction='mean') on soft targets (experiment_init.py:257-261, criterion "CE").
 * C == 1 is the binary head (n_classes == 2: ONE logit, MTUNetPlusPlus.py:39-41): ce_i = BCEWithLogits(x_i, t_i) =
 *   (1 - t) x + softplus(-x), target (N,1) in {0,1}; alpha = 1, gamma = 0 = torch.nn.BCEWithLogitsLoss() (experiment_init.py:241-242). */
typedef struct {
    int32_t N, C;
    float alpha, gamma;
    const float* x; const float* target; const float* weight;   /* weight may be NULL */
    float* loss;                     /* 1 float */
    float* dx;                       /* (N,C) or NULL */
    float gscale;
    const float* gscale_dev;
} mtbc_focal_args;
int mtbc_focal_fwd_bwd(const mtbc_focal_args* a, void* stream);

/* -------------------------------------------------------------- loss mix + NaN guard
 * replaces training_multitask.py:98 (alpha-mix) and the isnan guard of criterions.py:72-76:
 *   out[0] = alpha*seg + (1-alpha)*cls, out[1] = seg, out[2] = cls, out[3] = nan flag (0/1)  */
int mtbc_loss_mix(const float* seg, const float* cls, float alpha, float* out4, void* stream);

/* -------------------------------------------------------------- softmax over the rows of (N, C) logits, C <= 3
 * The output nn.Softmax(dim=1) of the single-task classifier (nnUNet_classifier.py:168-169), which the reference's criterion then reads as if
 * the probabilities were logits.  backward == 0: p = exp(x - max x) / sum exp(x - max x), the max-subtracted form torch evaluates (an all -inf
 * row gives NaN as it does there).  backward != 0: dz = p * (dp - sum_c p_c dp_c) from the forward's p.  One block; a thread owns whole rows,
 * so there is no reduction across threads.  exp is the library's own (range reduction by ln 2 in two pieces, degree-7 polynomial, fused
 * multiply-adds written out, no contraction): the row function is compiled once for host and device and gives the same bits on both.
 * mtbc_softmax_rows_host: the same function on host pointers, no GPU call.  dz may alias dp.
 * MTBC_E_BADSHAPE: N < 1 or C outside 1 .. 3; MTBC_E_BADARG: a null pointer the direction reads or writes.                                   */
typedef struct {
    int32_t N, C;
    int32_t backward;                /* 0: x -> p; else (p, dp) -> dz */
    const float* x;                  /* (N, C) logits (forward) */
    float* p;                        /* (N, C) probabilities: written by the forward, read by the backward */
    const float* dp;                 /* (N, C) d loss / d p (backward) */
    float* dz;                       /* (N, C) d loss / d x (backward) */
} mtbc_softmax_args;
int mtbc_softmax_rows(const mtbc_softmax_args* a, void* stream);
int mtbc_softmax_rows_host(const mtbc_softmax_args* a);

/* ------------------------------------------------------------------------------------ dynamic loss scale
 * torch.amp.GradScaler's rule, stream-ordered on the device (no host read in the step).  One step is
 *   mtbc_loss_scale_begin -> forward, losses, backward [, all-reduce] -> mtbc_loss_scale_check -> mtbc_loss_scale_optim
 * The state is 64 bytes of DEVICE memory owned by the caller (zero-filled, then `scale` set); every field is written by ordinary
 * vector stores / atomics, kernel boundaries order them.                                                                        */
typedef struct {
    float    scale;                  /* the loss scale: a power of two as long as the factors are */
    int32_t  growth_tracker;         /* clean steps since the scale last changed */
    uint32_t found_inf;              /* set by _check when a gradient is inf / NaN, cleared by _optim's update */
    int32_t  t;                      /* Adam updates actually APPLIED (a skipped step does not count) */
    int32_t  skipped;                /* steps skipped so far */
    float    lr;                     /* the caller writes the learning rate of the step here, in stream order, before _begin */
    float    shard_weight;           /* the caller's factor on dL (1, or this rank's share of an unequal global batch times world) */
    float    adam[3];                /* _begin: {inv_world / scale, lr / (1-b1^(t+1)), 1 / sqrt(1-b2^(t+1))} = the first three words of mtbc_optim_args.dynamic for that step */
    int32_t  reserved[6];
} mtbc_loss_scale_state;
typedef struct {
    mtbc_loss_scale_state* state;    /* DEVICE memory (HOST memory for mtbc_loss_scale_update_host), 4-byte aligned */
    float* gscale_out;               /* _begin: *gscale_out = shard_weight * scale -- the word mtbc_dice_args / mtbc_focal_args.gscale_dev point at */
    const float* g; int64_t n;       /* _check: the flat gradient buffer (16-byte aligned), every element of [0, n) is read */
    double growth_factor, backoff_factor;      /* the scale is multiplied in double and rounded once, as torch._amp_update_scale_ does */
    int32_t growth_interval;         /* >= 1 */
    float inv_world;                 /* 1 / world size: Adam's grad_scale is inv_world / scale */
    float beta1, beta2;              /* the bias corrections of step t + 1 are evaluated on the device, in double */
} mtbc_loss_scale_args;
/* one thread: the loss kernels' device factor and Adam's three scalars for the step that follows (state->t + 1) */
int mtbc_loss_scale_begin(const mtbc_loss_scale_args* a, void* stream);
/* one streaming pass over g (float4 loads, grid-stride, grid sized like mtbc_optim_step's): found_inf = 1 when any element has an all-ones exponent */
int mtbc_loss_scale_check(const mtbc_loss_scale_args* a, void* stream);
/* host only, no GPU call: the update rule of mtbc_loss_scale_optim (below) on a HOST copy of the state (the device kernel runs the same inline function):
 *   found_inf: scale *= backoff_factor, growth_tracker = 0, skipped += 1
 *   else     : t += 1, growth_tracker += 1, and at growth_interval: scale *= growth_factor (kept when that is not finite), growth_tracker = 0
 *   found_inf = 0                                                                                                               */
int mtbc_loss_scale_update_host(const mtbc_loss_scale_args* a);
/* host only: what _begin writes into state->adam for the `t`, `scale` and `lr` of a HOST copy of the state */
int mtbc_loss_scale_begin_host(const mtbc_loss_scale_args* a);

/* ------------------------------------------------------------------------------------ Adam, SGD (Nesterov) and AdamW
 * replaces torch.optim.Adam(lr, betas=(.9,.999), eps=1e-4).step(), torch.optim.SGD(lr, momentum=0.9, nesterov=True).step() and
 * torch.optim.AdamW(lr).step() of experiment_init.py:186-195, training_multitask.py:103 -- one fused launch over the flat parameter buffer.
 *   g' = grad_scale * g
 *   SGD   : buf = momentum buf + g' ; d = nesterov ? g' + momentum buf : buf ; p -= lr d            (dampening 0, weight_decay 0; buf starts at 0)
 *   AdamW : p *= (float)(1 - (double)lr (double)weight_decay) ;
 *           m = m + (1-b1)(g'-m) ; v = b2 v + (1-b2) g'^2 ; p -= (lr / (1-b1^t)) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
 *   Adam  : kind = MTBC_OPT_ADAMW with weight_decay = 0 -- the decay factor is then exactly 1.0f and p * 1.0f is p.  There is no third kind and
 *           no Adam struct or entry point of its own (there was until version 202; the words that kernel wrote are what this one writes).
 * Every element goes through ONE inline function compiled for host and device without floating-point contraction (the fused operations are
 * spelled fmaf), so mtbc_optim_step_host gives the kernel's bits.  v is fma(g', (1-b2) g', b2 v) on the elements below n & ~3 and the two
 * products summed on the rest (at most three elements; none when n is a multiple of four).                                                  */
#define MTBC_OPT_SGD   0
#define MTBC_OPT_ADAMW 1
typedef struct {
    int32_t kind;                    /* MTBC_OPT_SGD | MTBC_OPT_ADAMW */
    int64_t n;
    float* p; const float* g;
    float* m;                        /* SGD: the momentum buffer; AdamW: exp_avg */
    float* v;                        /* AdamW: exp_avg_sq; SGD: not read (may be NULL) */
    float lr, beta1, beta2, eps, momentum, weight_decay, grad_scale;
    int32_t step;                    /* t >= 1 (AdamW's bias corrections; SGD does not use it) */
    int32_t zero_grad;               /* 1 = also clear g */
    int32_t nesterov;                /* SGD */
    const float* dynamic;            /* optional, DEVICE memory, 4 floats as mtbc_optim_dynamic writes them: read instead of lr / step / grad_scale
                                        (a step replayed as a hipGraph).  NULL: the launch arguments.  Same arithmetic, same bits. */
    const uint32_t* skip;            /* optional: a found-inf word.  Non-zero: every thread returns before touching p / m / v (zero_grad still clears g) */
    const mtbc_loss_scale_state* scale_state;   /* optional: the scalars come from a dynamic loss scale's state instead -- grad_scale = adam[0],
                                        AdamW: adam[1], adam[2] and the decay factor from state->lr, SGD: lr = state->lr.  Goes before `dynamic`. */
} mtbc_optim_args;
/* 16-byte alignment of p, g, m (and v for AdamW) required, else MTBC_E_UNSUPPORTED.  Grid-stride, float4 body and a scalar tail. */
int mtbc_optim_step(const mtbc_optim_args* a, void* stream);
/* host only, no GPU call: out4 = {grad_scale, SGD: lr | AdamW: lr / (1-b1^t), AdamW: 1 / sqrt(1-b2^t) | SGD: 1,
 *                                 AdamW: (float)(1 - (double)lr (double)weight_decay) | SGD: 1}, bias corrections in double as torch.optim.Adam's scalar path */
int mtbc_optim_dynamic(const mtbc_optim_args* a, float out4[4]);
/* the last launch of a step under the dynamic loss scale: mtbc_optim_step(opt) with skip = &state->found_inf and scale_state = state -- every
 * thread returns before touching p / m / v when found_inf is set (zero_grad still clears g) -- then one thread applies the update rule (see
 * mtbc_loss_scale_update_host) to the state and clears found_inf.  `opt->lr`, `step`, `grad_scale`, `dynamic`, `skip` and `scale_state` are not
 * read.  SGD ignores state->adam[1..2].  Two launches, no grid-wide barrier.                                                              */
int mtbc_loss_scale_optim(const mtbc_loss_scale_args* a, const mtbc_optim_args* opt, void* stream);
/* host only, no GPU call: the same update on HOST pointers (p, g, m, v, and dynamic / skip / scale_state where set), a plain loop over the
 * inline element function the kernel runs. */
int mtbc_optim_step_host(const mtbc_optim_args* a);

/* Whole-batch TP/FP/FN of (sigmoid(x) > .5) vs target, the train-loop Dice metric of
 * metrics.py:255-267 (training_multitask.py:66-71).  out3 = {tp, fp, fn} as float64.        */
int mtbc_dice_counts(const float* logits, const float* target, int64_t n, double* out3, void* stream);

/* ------------------------------------------------------------------ per-image test-phase metrics
 * The integer table behind `results_segmentation.csv` / `results_classification.csv` of the testing phase
 * (utils/models.py:273-397; metrics.py:26-74 calculate_metrics, :238-252 haussdorf_distance; images.py:41-55): one row of
 * MTBC_SEGM_COLS int64 values per image, every one exact.  In the reference's order: raw mask = sigmoid(seg_logits) > .5 (the
 * predicate of the Dice counters above); pixel_threshold > 0 and raw_pixels <= pixel_threshold clears the mask; seg_from_class
 * and cls_raw == normal_class clears the mask; cls_final = normal_class when class_from_seg and raw_pixels == 0 (the RAW count),
 * else cls_raw.  The two class rules need n_cls >= 2: the binary head (n_cls == 1, cls = sigmoid > .5) has none (:186-270).
 *   hd_rows_sq  the square of what the reference reports as "Haussdorf distance": scipy's directed_hausdorff takes each image ROW
 *               as one point, so it is max over rows of one mask of the smallest Hamming distance to a row of the other (both ways)
 *   hd_px_sq    the squared Hausdorff distance between the two pixel sets, over every pixel of each set
 *   both: 0 when both masks are empty, -1 when exactly one is (the reference gives NaN).
 * H and W: multiples of 16 in [16, 512].  Two launches on `stream`; `out` and `workspace` need no initialisation and are 8-byte
 * aligned; results are bit-reproducible (integer atomics only).                                                          */
#define MTBC_SEGM_COLS 9
#define MTBC_SEGM_TP 0               /* tp, tn, fp, fn of the FINAL predicted mask against the target */
#define MTBC_SEGM_TN 1
#define MTBC_SEGM_FP 2
#define MTBC_SEGM_FN 3
#define MTBC_SEGM_RAW_PIXELS 4       /* tumour pixels of the raw prediction */
#define MTBC_SEGM_HD_ROWS_SQ 5
#define MTBC_SEGM_HD_PX_SQ 6
#define MTBC_SEGM_CLS_RAW 7          /* argmax of cls_logits (first maximum); -1 without cls_logits */
#define MTBC_SEGM_CLS_FINAL 8
typedef struct {
    int32_t N, H, W, n_cls;          /* n_cls: columns of cls_logits (1 .. 64), unread when cls_logits is NULL */
    const float* seg_logits;         /* (N,1,H,W) logits of the last segmentation head */
    const float* target;             /* (N,1,H,W) mask, != 0 is tumour */
    const float* cls_logits;         /* (N,n_cls) or NULL */
    int32_t pixel_threshold, seg_from_class, class_from_seg, normal_class;
    int64_t* out;                    /* (N, MTBC_SEGM_COLS) */
    void* workspace; size_t workspace_bytes;
} mtbc_seg_metrics_args;
/* host only, no GPU call; 0 for a shape the call refuses */
size_t mtbc_seg_metrics_workspace_size(const mtbc_seg_metrics_args* a);
int mtbc_seg_metrics(const mtbc_seg_metrics_args* a, void* stream);

/* ------------------------------------------------------------------ training-time metrics
 * The counts behind the Train_dice / Train_acc / Train_F1 columns of the reference's epoch loop (training_multitask.py:105-113),
 * appended on the device by a call that sits between a step's loss ops and its backward ops (the backward reuses the outputs'
 * memory).  Two stream-ordered launches, no host involvement, integer atomics only (bit-reproducible):
 *   pixels   tp / fp / fn of (sigmoid(seg_logits) > .5 -- the predicate of the Dice counters above) against mask != 0 over the
 *            WHOLE batch (process_segmentation_predicted, :65-71), added to table[cursor][0..2]
 *   samples  predicted class = first maximum of the logits row, a NaN counting as the maximum (torch.argmax of the softmax,
 *            :41-46), true class = first maximum of the target row; n_logits == 1: sigmoid(logit) > .5 against target != 0
 *            (:53-61).  conf[true][predicted] += 1, table[cursor][3] += N, then cursor += 1.
 * The row index lives in device memory (state[0]) because a replayed hipGraph holds fixed arguments.  With cursor >= capacity
 * nothing is added to `table` or `conf`; state[1] counts such calls (with N > 0) and the cursor still advances.  N == 0 with
 * n_seg == 0 is the empty shard of a data-parallel rank: the cursor advances and nothing else happens, so that row b is global
 * batch b on every rank (the data pointers may then be NULL).  The caller zeroes table, conf and state before the first call.
 * MTBC_E_BADARG: a null pointer; MTBC_E_BADSHAPE: n_logits outside 1 .. 3, a negative count, N == 0 without n_seg == 0.     */
typedef struct {
    const float* seg_logits;         /* last segmentation head, fp32, n_seg = N*C*H*W elements */
    const float* mask;               /* the step's mask buffer, same element count */
    int64_t      n_seg;
    const float* cls_logits;         /* (N, n_logits) fp32 */
    const float* target;             /* (N, n_logits): one-hot rows, or the {0,1} label when n_logits == 1 */
    int32_t      N, n_logits;
    int64_t*     table;              /* [capacity][4]: tp, fp, fn, samples -- one row per batch */
    int64_t*     conf;               /* [3][3] rows = ground truth, cols = prediction */
    int32_t*     state;              /* [0] cursor = batches seen, [1] batches dropped (cursor >= capacity) */
    int32_t      capacity;
} mtbc_train_metrics_args;
int mtbc_train_metrics(const mtbc_train_metrics_args* a, void* stream);

/* ---- validation-epoch metrics (training_multitask.py:119-159): mtbc_train_metrics' two launches -- the same pixel kernel and predicate, the
 * same sample rule, the same cursor, capacity and drop counter, the same integer atomics -- plus the batch's loss words recorded in the row
 * the call appends.  With the row in range and N > 0, one thread of the samples launch stores
 *   loss_rows[cursor][0..3] = w * (double)loss_in[0..3]
 * before the cursor advances: loss_in = the step's [total, seg, cls, nan_flag] words, w = *shard_weight, a word in DEVICE memory that
 * the host fills in stream order in front of the call (a replayed hipGraph holds fixed arguments and reads the value of the day);
 * shard_weight == NULL means 1.  Plain stores, no floating-point atomic: bit-reproducible.  With cursor >= capacity nothing is written
 * anywhere and state[1] counts the call; the empty shard (N == 0 with n_seg == 0) advances the cursor and writes nothing, so with
 * loss_rows zeroed beforehand (as table, conf and state are) the sum of the ranks' row b is the sum over the ranks that had samples.
 * MTBC_E_BADARG: a null pointer -- loss_in and loss_rows may be NULL only with N == 0, as the data pointers; MTBC_E_BADSHAPE: as
 * mtbc_train_metrics.  The first eleven fields are mtbc_train_metrics_args'.                                                       */
typedef struct {
    const float* seg_logits;
    const float* mask;
    int64_t      n_seg;
    const float* cls_logits;
    const float* target;
    int32_t      N, n_logits;
    int64_t*     table;
    int64_t*     conf;
    int32_t*     state;
    int32_t      capacity;
    const float* loss_in;            /* 4 floats: total, seg, cls, nan_flag of the batch */
    double*      loss_rows;          /* [capacity][4] */
    const float* shard_weight;       /* device word n_local / n_batch of this rank, or NULL = 1 */
} mtbc_eval_metrics_args;
int mtbc_eval_metrics(const mtbc_eval_metrics_args* a, void* stream);

/* ---- metrics of a segmentation-only step (training_segmentation.py:40-88): the pixel launch of mtbc_train_metrics -- the same kernel, the same
 * predicate -- then a ONE-thread launch that adds N to table[cursor][3], stores loss_rows[cursor][0..3] = w * (double)loss_in[0..3] when loss_in
 * is not NULL (w = *shard_weight, NULL = 1), and advances the cursor.  Cursor and state, capacity and the drop counter, the empty shard
 * (N == 0 with n_seg == 0: only the cursor advances) behave exactly as in mtbc_eval_metrics; there are no class arguments and no confusion
 * matrix.  loss_in == NULL is the training call (loss_rows is then unread).  MTBC_E_BADARG: a null pointer (the data pointers may be NULL with
 * N == 0; loss_rows must be given with loss_in and N > 0); MTBC_E_BADSHAPE: a negative count, N == 0 without n_seg == 0.                       */
typedef struct {
    const float* seg_logits;         /* last segmentation head, fp32, n_seg = N*C*H*W elements */
    const float* mask;               /* the step's mask buffer, same element count */
    int64_t      n_seg;
    int32_t      N;
    int64_t*     table;              /* [capacity][4]: tp, fp, fn, samples -- one row per batch */
    int32_t*     state;              /* [0] cursor, [1] batches dropped */
    int32_t      capacity;
    const float* loss_in;            /* 4 floats [total, seg, 0, nan_flag] of the batch, or NULL */
    double*      loss_rows;          /* [capacity][4] */
    const float* shard_weight;       /* device word, or NULL = 1 */
} mtbc_seg_step_metrics_args;
int mtbc_seg_step_metrics(const mtbc_seg_step_metrics_args* a, void* stream);

/* ---- metrics of a classification-only step (training_classification.py:34-162): the samples launch of mtbc_train_metrics / mtbc_eval_metrics --
 * the same kernel, the same predicate on the model's OUTPUT (for a 3-class nnUNetClassifier that is the probabilities: first of equal maxima) --
 * and nothing else: conf[true][predicted] += 1 per sample, table[cursor][3] += N, loss_rows[cursor][0..3] = w * (double)loss_in[0..3] when
 * loss_in is not NULL (w = *shard_weight, NULL = 1), then the cursor advances.  There is no pixel launch: table[cursor][0..2] stay zero.
 * Cursor and state, capacity and the drop counter, the empty shard (N == 0: only the cursor advances) behave exactly as in
 * mtbc_seg_step_metrics.  MTBC_E_BADARG: a null pointer (the data pointers may be NULL with N == 0; loss_rows must be given with loss_in and
 * N > 0); MTBC_E_BADSHAPE: n_logits outside 1 .. 3, a negative count.                                                                        */
typedef struct {
    const float* cls_out;            /* (N, n_logits) fp32: what the model returns */
    const float* target;             /* (N, n_logits): one-hot rows, or the {0,1} label when n_logits == 1 */
    int32_t      N, n_logits;
    int64_t*     table;              /* [capacity][4]: 0, 0, 0, samples -- one row per batch */
    int64_t*     conf;               /* [3][3] rows = ground truth, cols = prediction */
    int32_t*     state;              /* [0] cursor, [1] batches dropped */
    int32_t      capacity;
    const float* loss_in;            /* 4 floats [cls, 0, cls, nan_flag] of the batch, or NULL */
    double*      loss_rows;          /* [capacity][4] */
    const float* shard_weight;       /* device word, or NULL = 1 */
} mtbc_cls_step_metrics_args;
int mtbc_cls_step_metrics(const mtbc_cls_step_metrics_args* a, void* stream);

/* ---- per-image rows of the classification driver's testing phase (utils/models.py:400-505): ONE launch of one block appends
 * (ground_truth, predicted_label) of each of the batch's N images to rows[cursor .. cursor + N) and advances the cursor by N.  The rule is the
 * samples rule above: first maximum of the output row against first maximum of the one-hot row; n_logits == 1: sigmoid(output) > .5 against
 * target != 0.  A batch that does not fit (cursor + N > capacity) writes nothing, adds 1 to state[1], and the cursor still advances.
 * MTBC_E_BADARG: a null pointer; MTBC_E_BADSHAPE: N < 1, n_logits outside 1 .. 3, a negative capacity.                                       */
typedef struct {
    const float* cls_out;            /* (N, n_logits) */
    const float* target;             /* (N, n_logits) one-hot, or (N, 1) {0,1} */
    int32_t      N, n_logits;
    int32_t*     rows;               /* [capacity][2]: ground truth, predicted label */
    int32_t*     state;              /* [0] cursor = images seen, [1] batches dropped */
    int32_t      capacity;
} mtbc_cls_test_rows_args;
int mtbc_cls_test_rows(const mtbc_cls_test_rows_args* a, void* stream);

/* ------------------------------------------------------------------ hole filling of a predicted mask
 * scipy.ndimage.binary_fill_holes (default structure) of the raw prediction, which the segmentation driver's testing phase applies before its
 * metrics (utils/models.py:39-100, fill_holes=True): foreground = sigmoid(seg_logits) > .5, the predicate of the Dice counters above (a NaN is
 * not foreground).  A non-foreground pixel is background-reachable when it lies on the image border or is 4-adjacent to a reachable
 * non-foreground pixel; the output is the complement of the reachable set, so an 8-connected ring encloses its interior.
 * One workgroup per image, both bit planes (free, reached) in LDS; a pass is four directional sweeps (r[i] |= r[i-1] & free[i] along rows both
 * ways, then along columns both ways), repeated until a pass sets no bit: deterministic, no atomics on global memory.  The pass loop is
 * bounded by H*W + 1 (every non-final pass sets a bit); reaching the bound stores 1 into *error and returns what it has -- *error is never
 * cleared by the call.  H, W: multiples of 16 in [16, 512], else MTBC_E_BADSHAPE; N >= 1.  At least one of the two outputs must be given.
 * mtbc_fill_holes_host: host pointers, no GPU call, the same pass and predicate code compiled for the host.                                 */
typedef struct {
    int32_t N, H, W;
    const float* seg_logits;         /* (N,1,H,W) */
    float*   filled_logits;          /* (N,1,H,W): +1.f foreground after filling, -1.f otherwise; or NULL */
    uint8_t* filled_u8;              /* (N,H,W): 255 / 0; or NULL */
    int32_t* error;                  /* one word */
} mtbc_fill_holes_args;
int mtbc_fill_holes(const mtbc_fill_holes_args* a, void* stream);
int mtbc_fill_holes_host(const mtbc_fill_holes_args* a);

/* ---------------------------------------------------------------------------- step program
 * A training step is a static list of the ops above with every pointer resolved at plan
 * time; mtbc_program_run issues them back-to-back on one stream (no host work in between). */
enum {
    MTBC_OP_CONV3_FWD = 1, MTBC_OP_CONV3_DGRAD, MTBC_OP_CONV3_WGRAD,
    MTBC_OP_CONV3_PACK_FWD, MTBC_OP_CONV3_PACK_DGRAD,
    MTBC_OP_IN_FWD, MTBC_OP_IN_BWD, MTBC_OP_POOL_FWD, MTBC_OP_POOL_BWD,
    MTBC_OP_CONVT_FWD, MTBC_OP_CONVT_DGRAD, MTBC_OP_CONVT_WGRAD,
    MTBC_OP_CONV1_FWD, MTBC_OP_CONV1_DGRAD, MTBC_OP_CONV1_WGRAD,
    MTBC_OP_GAP_FWD, MTBC_OP_GAP_BWD, MTBC_OP_LINEAR_FWD, MTBC_OP_LINEAR_BWD,
    MTBC_OP_DICE_FWD, MTBC_OP_DICE_BWD, MTBC_OP_FOCAL, MTBC_OP_LOSS_MIX, MTBC_OP_OPTIM,
    MTBC_OP_MEMSET, MTBC_OP_DICE_COUNTS, MTBC_OP_CONV3_PACK_LP, MTBC_OP_HEAD_COMBINE, MTBC_OP_HEAD_EXPAND,
    MTBC_OP_C8_PACK, MTBC_OP_C8_PACK16, MTBC_OP_CONV3_WVIEW,
    MTBC_OP_SET_STREAM, MTBC_OP_EVENT_RECORD, MTBC_OP_EVENT_WAIT,
    MTBC_OP_IN_DPARAM
};
/* appended kinds (additive: the list above is as it was) */
enum { MTBC_OP_SOFTMAX = 37,         /* mtbc_softmax_rows on u.softmax, either direction */
       MTBC_OP_UPSAMPLE2_FWD = 38, MTBC_OP_UPSAMPLE2_BWD = 39 };      /* mtbc_upsample2_fwd / _bwd on u.up2 */
/* (the last three: stream control of mtbc_program_run_ms -- independent ops of a step, the weight gradient and the input
 * gradient of one layer, overlap on two HIP streams: the small latency-bound launches of the deep levels fill the chip together) */

/* ---- deep-supervision head of MTnnUNet: ConvTranspose2d(Cin->Cmid, k=s) followed by Conv2d(Cmid->R, 1x1)
 * (MTnnUNet.py:106-116: output4 k=8, output3 k=4, output2 k=2).  With no non-linearity in between the pair is ONE
 * transposed conv with Wc[ci][r][a][b] = sum_co wT[ci][co][a][b] * w1[r][co], bc[r] = sum_co bT[co] * w1[r][co] + b1[r]:
 * the Cmid x (kH x kW) intermediate (2.1 GB at B=64, k=8) and 128x the FLOPs disappear.  `combine` builds Wc / bc
 * (every step: the weights move), the ordinary mtbc_convT_{fwd,dgrad,wgrad} run with Cout = R, and `expand` maps the
 * gradient G of Wc and gb of bc back onto the four parameter tensors:
 *   dwT[ci][co][ab] = sum_r G[ci][r][ab] w1[r][co]        dbT[co] = sum_r gb[r] w1[r][co]
 *   dw1[r][co] = sum_{ci,ab} G[ci][r][ab] wT[ci][co][ab] + gb[r] bT[co]        db1[r] = gb[r]
 * Same function as the reference's two layers up to fp32 re-association (checked against the reference's goldens). */
typedef struct {
    int32_t Cin, Cmid, R, k;
    const float* wT; const float* bT;     /* (Cin,Cmid,k,k), (Cmid) */
    const float* w1; const float* b1;     /* (R,Cmid), (R)          */
    float* Wc; float* bc;                 /* (Cin,R,k,k), (R): written by combine */
    const float* G; const float* gb;      /* gradients of Wc / bc: read by expand  */
    float* dwT; float* dbT; float* dw1; float* db1;
    int32_t acc_wT, acc_bT, acc_w1, acc_b1;
} mtbc_head_fuse_args;
int mtbc_convT_head_combine(const mtbc_head_fuse_args* a, void* stream);
int mtbc_convT_head_expand(const mtbc_head_fuse_args* a, void* stream);

/* ---- training-time augmentation: RandomHorizontalFlip(.5) -> RandomVerticalFlip(.5) ->
 * RandomRotation(360) of training_multitask.py:193-197 / BUSI_dataset.py:142-147 on the joint (mask, image) stack,
 * torchvision semantics (nearest, zero fill, centre rotation).  src/dst (N,C,H,W), src != dst; params (N,4) =
 * {cos a, sin a, flip_h, flip_v} per sample, a = rotation angle (counter-clockwise, as torchvision's `angle`). */
int mtbc_augment_flip_rotate(const float* src, float* dst, const float* params, int32_t N, int32_t C, int32_t H, int32_t W,
                             void* stream);

/* ---- batch assembly from a device-resident uint8 dataset: ONE launch from a device index array to the fp32
 * input buffers of a step.  Sample n of the batch is store row index[n] (BUSI_dataset.py:97-158, training_multitask.py:82-84):
 *   out_image (N, 1 + K, H, W)   channel 0 = the raw image, channel 1 + k = luts[k][pixel] (the intensity variants of
 *                                `data.augmentation`, BUSI_dataset.py:123-139, in the reference's append order)
 *   out_mask  (N, 1, H, W)
 *   out_target                   n_onehot == 3: one-hot (N, 3) of the label; n_onehot == 0: the float label (N, 1) of the binary head
 * params (N, 4) = {cos a, sin a, flip_h, flip_v} per sample as for the augmentation call above, applied jointly to every plane
 * with the same source pixel and zero fill outside the rotated frame (the LUT planes too); NULL = identity (validation, test).
 * Every output element is written by this launch alone (no atomics, no workspace); any H, W > 0.  An index outside [0, M) never
 * reads the stores: that sample's planes and target are written as zeros.  MTBC_E_BADARG: a null pointer (luts may be NULL with
 * K == 0) or an output that overlaps another buffer; MTBC_E_BADSHAPE: a non-positive size, K outside [0, MTBC_BATCH_MAX_LUTS],
 * n_onehot outside {0, 3}.                                                                                                 */
#define MTBC_BATCH_MAX_LUTS 4
typedef struct {
    int32_t M, N, H, W;              /* store rows, batch size, plane size */
    int32_t K, n_onehot;             /* look-up tables (0 .. MTBC_BATCH_MAX_LUTS); 3 = one-hot target, 0 = float label */
    const uint8_t* images;           /* (M, H, W) */
    const uint8_t* masks;            /* (M, H, W), values {0, 1} */
    const int32_t* labels;           /* (M) */
    const int32_t* index;            /* (N) device array of store rows */
    const float* params;             /* (N, 4) or NULL */
    const uint8_t* luts;             /* (K, 256) */
    float* out_image; float* out_mask; float* out_target;
} mtbc_batch_args;
int mtbc_batch_assemble(const mtbc_batch_args* a, void* stream);

/* The same launch with E stored planes per image next to the image store: the spatial variants of `data.augmentation` (CLAHE, SOBEL:
 * BUSI_dataset.py:114-122), which are no function of the pixel value and are therefore data the caller computed once per image.
 *   out_image (N, 1 + E + K, H, W)   channel 0 = the raw image, channel 1 + e = planes[e] of the sample's store row, channel
 *                                    1 + E + k = luts[k][pixel] -- the reference's append order with CLAHE, SOBEL stored in that order
 * A stored plane is treated as the image plane is: row index[n], the same source pixel under params, 0 outside the rotated frame, 0 for
 * an index outside [0, M), the uint8 value converted to float.  Mask, target and LUT channels are those of mtbc_batch_assemble, and with
 * E == 0 every output word is.  Refused like mtbc_batch_assemble, plus MTBC_E_BADSHAPE: E outside [0, MTBC_BATCH_MAX_PLANES];
 * MTBC_E_BADARG: planes NULL with E > 0, or planes (E * M * H * W bytes) overlapping an output.                               */
#define MTBC_BATCH_MAX_PLANES 2
typedef struct {
    int32_t M, N, H, W;              /* store rows, batch size, plane size */
    int32_t K, n_onehot;             /* as in mtbc_batch_args */
    int32_t E;                       /* stored planes per image (0 .. MTBC_BATCH_MAX_PLANES) */
    const uint8_t* images;           /* (M, H, W) */
    const uint8_t* masks;            /* (M, H, W), values {0, 1} */
    const uint8_t* planes;           /* (E, M, H, W), one contiguous store */
    const int32_t* labels;           /* (M) */
    const int32_t* index;            /* (N) device array of store rows */
    const float* params;             /* (N, 4) or NULL */
    const uint8_t* luts;             /* (K, 256) */
    float* out_image; float* out_mask; float* out_target;
} mtbc_batch_planes_args;
int mtbc_batch_assemble_planes(const mtbc_batch_planes_args* a, void* stream);

typedef struct {
    int32_t kind;
    int32_t tag;                     /* free for the caller (layer id) */
    union {
        mtbc_conv3x3_args conv3;
        mtbc_instnorm_args inorm;
        mtbc_maxpool_args pool;
        mtbc_convT_args convT;
        mtbc_conv1x1_args conv1;
        mtbc_gap_args gap;
        mtbc_linear_args linear;
        mtbc_dice_args dice;
        mtbc_focal_args focal;
        mtbc_optim_args optim;
        struct { const float* w; float* packed; int32_t Cin, Cout; int32_t dgrad, compute; } pack;
        struct { const float* seg; const float* cls; float alpha; float* out4; } mix;
        struct { void* ptr; size_t bytes; } memset0;
        struct { const float* logits; const float* target; int64_t n; double* out3; } counts;
        mtbc_head_fuse_args head;
        struct { const float* w; float* dst; int32_t Cout, Cin, ci_off, ci_cnt, mode, k_off, K; } wview;
        struct { const float* src; int64_t src_batch_stride; void* dst; int32_t N, C, HW, compute; } c8pack;   /* C8_PACK and C8_PACK16 (src = 16-bit planar, `compute` unused) */
        mtbc_softmax_args softmax;
        mtbc_upsample2_args up2;
        mtbc_dparam_desc dparam;        /* MTBC_OP_IN_DPARAM: a run of them is issued as one mtbc_instnorm_dparam_many launch */
        struct { void* event; int32_t index; } sync;      /* SET_STREAM: following ops go to streams[index]; EVENT_RECORD / EVENT_WAIT: on the current stream */
    } u;
} mtbc_op;

/* run ops[first .. first+count) on `stream`; returns 0 or the first failing op's error code,
 * with *failed_index (may be NULL) set to its index. */
int mtbc_program_run(const mtbc_op* ops, int32_t first, int32_t count, void* stream, int32_t* failed_index);
/* The same with several streams: ops run on streams[0] until a MTBC_OP_SET_STREAM op selects another; MTBC_OP_EVENT_RECORD /
 * MTBC_OP_EVENT_WAIT order the streams (events from mtbc_event_create, reusable: a wait refers to the latest record issued
 * before it).  A range must begin and end on streams[0] with everything joined.  With n_streams == 1 every op runs on that
 * stream (indices are clamped): the same program, serialised.                                                            */
int mtbc_program_run_ms(const mtbc_op* ops, int32_t first, int32_t count, void* const* streams, int32_t n_streams, int32_t* failed_index);
/* timing-disabled HIP events for the two ops above; created when a step program is built, never inside a step */
int mtbc_event_create(void** event);
int mtbc_event_destroy(void* event);
/* Host-only plan query for the small ops: every launch the call behind op->kind would make for op->u, in order and joined with " + ",
 * written to buf (NUL-terminated).  Covers MTBC_OP_POOL_FWD / _BWD, MTBC_OP_CONV1_FWD / _DGRAD / _WGRAD, MTBC_OP_GAP_FWD / _BWD,
 * MTBC_OP_LINEAR_FWD / _BWD, MTBC_OP_UPSAMPLE2_FWD / _BWD, MTBC_OP_HEAD_COMBINE / _EXPAND and the ops of a step's loss program, MTBC_OP_DICE_FWD / _BWD,
 * MTBC_OP_FOCAL, MTBC_OP_LOSS_MIX and MTBC_OP_SOFTMAX; any other kind (the 3x3, InstanceNorm and ConvT ops have queries of their
 * own) is MTBC_E_BADARG.  Kernels are spelled as a profiler spells the instance without namespace and argument list, e.g.
 * "maxpool_c8_fwd_kernel<true>"; what the arguments select inside a kernel follows its name in brackets:
 *   conv1x1_c8_wgrad_kernel<F16> [nblk=1] | [nblk>1] | [nblk=32]   pixel chunks per image (one / several, the last may be ragged / the cap)
 *   plane_sum_k [threads=64] | [threads=256]                       the bias gradient's plane sums (256 from H*W = 4096)
 *   linear_dx_kernel [Out>=8], linear_dw_kernel [N>=8]             the eight-wide unrolled loop runs
 *   linear_wide_fwd_kernel + linear_wide_reduce_kernel             the batch-shared forward of a wide input and the sum of its split partials
 *   linear_wide_dx_kernel [+ linear_wide_dx_reduce_kernel]         ... its input gradient; the reduction only with more than one range of outputs
 *   upsample2_fwd_kernel | upsample2_fwd_scalar_kernel | upsample2_c8_fwd_kernel, upsample2_bwd_kernel | upsample2_bwd_scalar_kernel
 *   dice_stats_kernel<kind> [threads=256|1024 paths=vsvv rounds=0|=1|>1 rest part] + dice_finalize_kernel<kind> [planes>256]
 *                                                                  paths: per head the 16-byte (v) or the scalar (s) loop (H*W % 4 and the alignment of
 *                                                                  x[h] / target); then, for the 16-byte loop, the unrolled rounds of four loads a
 *                                                                  thread takes, `rest`: the loop behind them runs, `part`: some round or trip is taken by
 *                                                                  a part of the block only; [planes>256]: a finalize thread sums several planes
 *   dice_bwd_kernel<kind> [paths=vsvv loop]                        paths: as above, with dx[h]; loop: the grid is capped (4096 blocks) below a head's
 *                                                                  items, so the grid-stride loop takes a second trip
 *   focal_kernel [N>256], softmax_rows_kernel [N>64]               a thread of the one block owns more than one sample / row
 *   loss_mix_kernel
 * and the planar 1x1 weight gradient's reduction is named with its instance: "splitk_reduce<4>", "<16>" (more than 32 images) or
 * "<64, 16>" (256 images or more), e.g. "conv1x1_wgrad_kernel + splitk_reduce<4> + plane_sum_k [threads=64] + sum_over_n_k".
 * It is the dispatcher of the real call, stopped in front of its launches: launches nothing, never synchronises, needs no device and never
 * dereferences a tensor pointer (pointer VALUES count: NULL and alignment select branches); returns the code the real call would return
 * when it refuses the arguments, MTBC_E_BADARG for a NULL op or a buffer shorter than the name. */
int mtbc_op_kernel_name(const mtbc_op* op, char* buf, int32_t len);

#ifdef __cplusplus
}
#endif
#endif /* MTBC_H */
