// Training-time metrics of the reference's epoch loop (training_multitask.py:105-113) as integer counts appended on the device: one
// call reads what a step has just computed -- the last segmentation head, the mask, the classification logits and their target --
// and adds one row {tp, fp, fn, samples} to a persistent table plus the batch's cells to a 3 x 3 confusion matrix.  No host read, no
// host-written argument that changes from call to call: the row index is a cursor in device memory, so a replayed hipGraph (fixed
// kernel arguments) appends row after row.
//
// Two launches, not one with a last-arriver ticket: the pixel blocks all READ the cursor, the single sample block ADVANCES it as the
// last thing it does, and the kernel boundary between them is the ordering (a ticket needs device-scope release / acquire across
// the XCDs' L2s, measured 2.2 - 4 x slower on this chip: DESIGN.md section 3, round 4).
//
//   launch 1 (pixels)   grid-stride over n_seg (at most TM_MAX_BLOCKS blocks), 16-byte loads when both pointers are 16-byte aligned (the <= 3 elements behind the last
//                       whole vector and the unaligned case go through scalar loads of the same kernel).  Predicate sigmoidf_(x) > .5f
//                       of common.h -- ONE definition for the Dice loss, mtbc_dice_counts, mtbc_seg_metrics and this -- against
//                       mask != 0.  32-bit counters per thread and per wave, 64-bit from the block reduction (LDS) on, three 64-bit
//                       integer atomics per block into table[cursor].  cursor >= capacity: the block adds nothing.
//   launch 2 (samples)  one block: predicted / true class per sample into a 3 x 3 LDS tile, its non-zero cells added to `conf`, N added
//                       to table[cursor][3], cursor advanced (or, with the row out of range, the drop counter instead of the table).
// Integer atomics only: bit-reproducible.
//
// mtbc_eval_metrics (the validation epoch, training_multitask.py:119-159) is the same two launches with the batch's loss words recorded in the
// same row: the LOSS instantiation of the samples kernel has its thread 0 store loss_rows[cursor][0..3] = w * (double)loss_in[0..3] -- plain
// 8-byte vector stores, no floating-point atomic -- before it advances the cursor.  The instantiation mtbc_train_metrics launches carries none of it.
#include "common.h"

namespace {

constexpr int TM_BLOCK = 256;
constexpr int TM_WAVES = TM_BLOCK / MTBC_WAVE;
#ifndef TM_MAX_BLOCKS
#define TM_MAX_BLOCKS 256          // every block ends in three same-address atomics, and their number is what the launch costs (2048: 29 us, 256: 10 us): one block per CU
#endif
#ifndef TM_UNROLL
#define TM_UNROLL 4                // 16-byte load pairs a thread issues before it counts
#endif

__device__ __forceinline__ void count_pixel(float x, float t, unsigned& tp, unsigned& fp, unsigned& fn) {
    const bool s = sigmoidf_(x) > 0.5f, g = t != 0.f;
    tp += (s && g); fp += (s && !g); fn += (!s && g);
}

// VEC: x and t are 16-byte aligned.  A thread's 32-bit counters see about n / (gridDim * TM_BLOCK) pixels and a wave's 64 times that: the
// host refuses an n for which that could pass 2^32.
template <bool VEC>
__global__ __launch_bounds__(TM_BLOCK) void train_metrics_pixels_kernel(const float* __restrict__ x, const float* __restrict__ t, long long n,
                                                                         unsigned long long* __restrict__ table, const int* __restrict__ state,
                                                                         int capacity) {
    __shared__ unsigned long long red[TM_WAVES][3];
    const int cursor = state[0];                               // nobody writes this word during this launch
    if (cursor < 0 || cursor >= capacity) return;              // the table is full: the sample launch counts the drop
    unsigned tp = 0, fp = 0, fn = 0;
    const long long tid = (long long)blockIdx.x * TM_BLOCK + threadIdx.x, stride = (long long)gridDim.x * TM_BLOCK;
    long long done = 0;                                        // elements the vector body covers
    if (VEC) {
        const long long n4 = n >> 2;
        const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
        const f32x4* t4 = reinterpret_cast<const f32x4*>(t);
        long long i = tid;
        for (; i + (TM_UNROLL - 1) * stride < n4; i += TM_UNROLL * stride) {
            f32x4 xv[TM_UNROLL], tv[TM_UNROLL];
#pragma unroll
            for (int u = 0; u < TM_UNROLL; ++u) { xv[u] = x4[i + u * stride]; tv[u] = t4[i + u * stride]; }
#pragma unroll
            for (int u = 0; u < TM_UNROLL; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) count_pixel(xv[u][j], tv[u][j], tp, fp, fn);
        }
        for (; i < n4; i += stride) {
            const f32x4 xv = x4[i], tv = t4[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) count_pixel(xv[j], tv[j], tp, fp, fn);
        }
        done = n4 << 2;
    }
    for (long long i = done + tid; i < n; i += stride) count_pixel(x[i], t[i], tp, fp, fn);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { tp += __shfl_xor(tp, o, 64); fp += __shfl_xor(fp, o, 64); fn += __shfl_xor(fn, o, 64); }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { red[wid][0] = tp; red[wid][1] = fp; red[wid][2] = fn; }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < TM_WAVES; ++w) s += red[w][threadIdx.x];
        atomicAdd(&table[(size_t)cursor * 4 + threadIdx.x], s);
    }
}

// index of the first maximum of v[0 .. c), a NaN counting as the maximum (torch.argmax)
__device__ __forceinline__ int first_argmax(const float* v, int c) {
    int best = 0;
    float bv = v[0];
    for (int i = 1; i < c; ++i) {
        const float u = v[i];
        if (bv == bv && (u != u || u > bv)) { best = i; bv = u; }      // a NaN already held stays: the first one wins
    }
    return best;
}

// LOSS: the evaluation call -- loss_in = the plan's [total, seg, cls, nan_flag] words, w = *shard_weight (NULL: 1), loss_rows [capacity][4]
template <bool LOSS>
__global__ __launch_bounds__(TM_BLOCK) void train_metrics_samples_kernel(const float* __restrict__ logits, const float* __restrict__ target, int N,
                                                                          int n_logits, unsigned long long* __restrict__ table,
                                                                          unsigned long long* __restrict__ conf, int* __restrict__ state,
                                                                          int capacity, const float* __restrict__ loss_in,
                                                                          double* __restrict__ loss_rows, const float* __restrict__ shard_weight) {
    __shared__ unsigned int tile[9];
    if (threadIdx.x < 9) tile[threadIdx.x] = 0u;
    __syncthreads();
    const int cursor = state[0];
    const bool in_range = cursor >= 0 && cursor < capacity;
    for (int s = threadIdx.x; s < N; s += TM_BLOCK) {
        int pred, gt;
        if (n_logits == 1) {                                   // binary head: training_multitask.py:53-61
            pred = sigmoidf_(logits[s]) > 0.5f ? 1 : 0;
            gt = target[s] != 0.f ? 1 : 0;
        } else {                                               // argmax of the softmax (monotone) against argmax of the one-hot row, :41-46
            pred = first_argmax(logits + (size_t)s * n_logits, n_logits);
            gt = first_argmax(target + (size_t)s * n_logits, n_logits);
        }
        atomicAdd(&tile[gt * 3 + pred], 1u);
    }
    __syncthreads();
    // `conf` describes exactly the batches that have a row in the table: a dropped batch adds to neither
    if (in_range && threadIdx.x < 9 && tile[threadIdx.x] != 0u) atomicAdd(&conf[threadIdx.x], (unsigned long long)tile[threadIdx.x]);
    if (threadIdx.x == 0) {
        if (N > 0) {
            if (in_range) {
                atomicAdd(&table[(size_t)cursor * 4 + 3], (unsigned long long)N);
                if (LOSS) {                                    // this row is this call's alone: plain stores
                    const double w = shard_weight ? (double)shard_weight[0] : 1.0;
                    double* row = loss_rows + (size_t)cursor * 4;
#pragma unroll
                    for (int j = 0; j < 4; ++j) row[j] = w * (double)loss_in[j];
                }
            } else state[1] += 1;
        }
        state[0] = cursor + 1;                                 // the last thing this call does to the cursor: the next call's launches read it
    }
}

// the pixels launch of every entry point of this file (n_seg == 0: none)
int launch_pixels(const float* seg_logits, const float* mask, int64_t n_seg, unsigned long long* table, const int32_t* state, int capacity, hipStream_t st) {
    if (n_seg > 0) {
        const long long n = (long long)n_seg;
        // memory-bound and small: one unrolled pass per thread before another block is added; past 2^40 pixels a wave's 32-bit counters
        // could wrap
        if (n >= (1ll << 40)) return MTBC_E_BADSHAPE;
        long long blocks = cdiv64(n, (long long)TM_BLOCK * 4 * TM_UNROLL);
        if (blocks > TM_MAX_BLOCKS) blocks = TM_MAX_BLOCKS;
        const bool vec = (uintptr_t)seg_logits % 16 == 0 && (uintptr_t)mask % 16 == 0;
        if (vec) hipLaunchKernelGGL(train_metrics_pixels_kernel<true>, dim3((unsigned)blocks), dim3(TM_BLOCK), 0, st, seg_logits, mask, n, table,
                                    (const int*)state, capacity);
        else hipLaunchKernelGGL(train_metrics_pixels_kernel<false>, dim3((unsigned)blocks), dim3(TM_BLOCK), 0, st, seg_logits, mask, n, table,
                                (const int*)state, capacity);
        MTBC_CHECK_LAUNCH();
    }
    return MTBC_OK;
}

// mtbc_seg_step_metrics' second launch, ONE thread: what thread 0 of the samples kernel does behind its class counts (loss_in NULL: no loss row)
__global__ void seg_step_tail_kernel(int N, unsigned long long* __restrict__ table, int* __restrict__ state, int capacity,
                                     const float* __restrict__ loss_in, double* __restrict__ loss_rows, const float* __restrict__ shard_weight) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int cursor = state[0];
    if (N > 0) {
        if (cursor >= 0 && cursor < capacity) {
            atomicAdd(&table[(size_t)cursor * 4 + 3], (unsigned long long)N);
            if (loss_in) {                                     // this row is this call's alone: plain stores
                const double w = shard_weight ? (double)shard_weight[0] : 1.0;
                double* row = loss_rows + (size_t)cursor * 4;
#pragma unroll
                for (int j = 0; j < 4; ++j) row[j] = w * (double)loss_in[j];
            }
        } else state[1] += 1;
    }
    state[0] = cursor + 1;
}

// both entry points: the argument checks they share, the pixels launch, then the samples launch of the caller's instantiation
template <bool LOSS>
int launch_metrics(const float* seg_logits, const float* mask, int64_t n_seg, const float* cls_logits, const float* target, int N, int n_logits,
                   int64_t* table_, int64_t* conf, int32_t* state, int capacity, const float* loss_in, double* loss_rows, const float* shard_weight,
                   void* stream) {
    if (!table_ || !conf || !state) return MTBC_E_BADARG;
    if (N < 0 || n_seg < 0 || capacity < 0 || n_logits < 1 || n_logits > 3) return MTBC_E_BADSHAPE;
    if ((N == 0) != (n_seg == 0)) return MTBC_E_BADSHAPE;                        // an empty shard has neither samples nor pixels
    if (N > 0 && (!seg_logits || !mask || !cls_logits || !target)) return MTBC_E_BADARG;
    if (LOSS && N > 0 && (!loss_in || !loss_rows)) return MTBC_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* table = reinterpret_cast<unsigned long long*>(table_);
    const int rc = launch_pixels(seg_logits, mask, n_seg, table, state, capacity, st);
    if (rc != MTBC_OK) return rc;
    hipLaunchKernelGGL(train_metrics_samples_kernel<LOSS>, dim3(1), dim3(TM_BLOCK), 0, st, cls_logits, target, N, n_logits, table,
                       reinterpret_cast<unsigned long long*>(conf), state, capacity, loss_in, loss_rows, shard_weight);
    MTBC_CHECK_LAUNCH();
    return MTBC_OK;
}

// mtbc_cls_test_rows: one block; sample s of the batch becomes row cursor + s = (ground truth, predicted label) by the samples rule above
__global__ __launch_bounds__(TM_BLOCK) void cls_test_rows_kernel(const float* __restrict__ out, const float* __restrict__ target, int N, int n_logits,
                                                                  int* __restrict__ rows, int* __restrict__ state, int capacity) {
    const int cursor = state[0];
    const bool fits = cursor >= 0 && N <= capacity && cursor <= capacity - N;
    if (fits)
        for (int s = threadIdx.x; s < N; s += TM_BLOCK) {
            int pred, gt;
            if (n_logits == 1) {
                pred = sigmoidf_(out[s]) > 0.5f ? 1 : 0;
                gt = target[s] != 0.f ? 1 : 0;
            } else {
                pred = first_argmax(out + (size_t)s * n_logits, n_logits);
                gt = first_argmax(target + (size_t)s * n_logits, n_logits);
            }
            rows[2 * ((size_t)cursor + s)] = gt;
            rows[2 * ((size_t)cursor + s) + 1] = pred;
        }
    __syncthreads();                                           // every thread has read the cursor
    if (threadIdx.x == 0) {
        if (!fits) state[1] += 1;
        if (cursor <= 0x7fffffff - N) state[0] = cursor + N;
    }
}

}  // namespace

extern "C" int mtbc_train_metrics(const mtbc_train_metrics_args* a, void* stream) {
    if (!a) return MTBC_E_BADARG;
    return launch_metrics<false>(a->seg_logits, a->mask, a->n_seg, a->cls_logits, a->target, a->N, a->n_logits, a->table, a->conf, a->state,
                                 a->capacity, nullptr, nullptr, nullptr, stream);
}

extern "C" int mtbc_eval_metrics(const mtbc_eval_metrics_args* a, void* stream) {
    if (!a) return MTBC_E_BADARG;
    return launch_metrics<true>(a->seg_logits, a->mask, a->n_seg, a->cls_logits, a->target, a->N, a->n_logits, a->table, a->conf, a->state,
                                a->capacity, a->loss_in, a->loss_rows, a->shard_weight, stream);
}

extern "C" int mtbc_seg_step_metrics(const mtbc_seg_step_metrics_args* a, void* stream) {
    if (!a) return MTBC_E_BADARG;
    if (!a->table || !a->state) return MTBC_E_BADARG;
    if (a->N < 0 || a->n_seg < 0 || a->capacity < 0) return MTBC_E_BADSHAPE;
    if ((a->N == 0) != (a->n_seg == 0)) return MTBC_E_BADSHAPE;                  // an empty shard has neither samples nor pixels
    if (a->N > 0 && (!a->seg_logits || !a->mask)) return MTBC_E_BADARG;
    if (a->N > 0 && a->loss_in && !a->loss_rows) return MTBC_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* table = reinterpret_cast<unsigned long long*>(a->table);
    const int rc = launch_pixels(a->seg_logits, a->mask, a->n_seg, table, a->state, a->capacity, st);
    if (rc != MTBC_OK) return rc;
    hipLaunchKernelGGL(seg_step_tail_kernel, dim3(1), dim3(1), 0, st, a->N, table, a->state, a->capacity, a->loss_in, a->loss_rows, a->shard_weight);
    MTBC_CHECK_LAUNCH();
    return MTBC_OK;
}

extern "C" int mtbc_cls_step_metrics(const mtbc_cls_step_metrics_args* a, void* stream) {
    if (!a) return MTBC_E_BADARG;
    if (!a->table || !a->conf || !a->state) return MTBC_E_BADARG;
    if (a->N < 0 || a->capacity < 0 || a->n_logits < 1 || a->n_logits > 3) return MTBC_E_BADSHAPE;
    if (a->N > 0 && (!a->cls_out || !a->target)) return MTBC_E_BADARG;
    if (a->N > 0 && a->loss_in && !a->loss_rows) return MTBC_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* table = reinterpret_cast<unsigned long long*>(a->table);
    unsigned long long* conf = reinterpret_cast<unsigned long long*>(a->conf);
    if (a->loss_in) hipLaunchKernelGGL(train_metrics_samples_kernel<true>, dim3(1), dim3(TM_BLOCK), 0, st, a->cls_out, a->target, a->N, a->n_logits, table,
                                       conf, a->state, a->capacity, a->loss_in, a->loss_rows, a->shard_weight);
    else hipLaunchKernelGGL(train_metrics_samples_kernel<false>, dim3(1), dim3(TM_BLOCK), 0, st, a->cls_out, a->target, a->N, a->n_logits, table,
                            conf, a->state, a->capacity, nullptr, nullptr, nullptr);
    MTBC_CHECK_LAUNCH();
    return MTBC_OK;
}

extern "C" int mtbc_cls_test_rows(const mtbc_cls_test_rows_args* a, void* stream) {
    if (!a) return MTBC_E_BADARG;
    if (!a->cls_out || !a->target || !a->rows || !a->state) return MTBC_E_BADARG;
    if (a->N < 1 || a->capacity < 0 || a->n_logits < 1 || a->n_logits > 3) return MTBC_E_BADSHAPE;
    hipLaunchKernelGGL(cls_test_rows_kernel, dim3(1), dim3(TM_BLOCK), 0, (hipStream_t)stream, a->cls_out, a->target, a->N, a->n_logits, a->rows,
                       a->state, a->capacity);
    MTBC_CHECK_LAUNCH();
    return MTBC_OK;
}
