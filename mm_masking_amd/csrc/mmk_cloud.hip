// Operations on whole point clouds, gfx950.  mmk_voxel_downsample: one output row per occupied cell of
// a uniform grid, in the order of first appearance, as the centroid of the cell's rows or as its first row.
//
// Four phases, each a kernel boundary (no tickets, no fences: DESIGN.md §8 item 4):
//   insert      one thread per row: the row's cell as one 64-bit key into a per-pair open-addressing table (atomicCAS, linear
//               probing, at most `cap` steps; cap = power of two >= 2 M, so a free slot always exists), atomicMin of the row
//               index and atomicAdd of the member count on the slot, atomicMax of the bits of max|value| per pair;
//   leaders     a row leads its cell when the slot's minimum is its own index; block counts, one scan per pair, ranks: the
//               stable compaction of the leaders in index order gives every slot its rank and the pair its count;
//   accumulate  one thread per (row, column): llrint(value · scale) added to (rank, column) with 64-bit integer atomics,
//               and voxel_of;
//   finalise    one thread per output row: the division, the normal, the padding fill, out_n and out_first.
// Integer atomics alone carry state between blocks inside a kernel, and only ever on the same words (CAS on a key, min /
// add on a counter): every result is independent of the arrival order.  No per-thread array is indexed at run time (no
// scratch memory: tests/test_code_objects.py); the columns are read from global memory.
#include <math.h>

#include "mmk_common.h"

namespace {

constexpr int VOX_THREADS = 256;
constexpr int VOX_WAVES = VOX_THREADS / 64;
constexpr unsigned long long VOX_EMPTY = ~0ull;               // a free slot (above every key: VOX_SPAN^3 < 2^64 − 1)
constexpr int VOX_HALF = 1 << 20;                             // cells −2^20 .. 2^20 per axis
constexpr unsigned long long VOX_SPAN = (1ull << 21) + 1ull;  // values of i_c + 2^20
constexpr int VOX_MAX_M = 1 << 28;                            // cap <= 2^29 fits an int

inline int vox_cap(int M)
{
    int cap = 2;
    while (cap < 2 * M) cap <<= 1;
    return cap;
}

inline int vox_blocks(int M) { return (M + VOX_THREADS - 1) / VOX_THREADS; }
inline int vox_lanes(int cols) { return cols <= 2 ? 2 : cols <= 4 ? 4 : 8; }      // lanes per row of the accumulate kernel

// Exclusive prefix sum of v over the block's VOX_THREADS threads (thread order) and the block's total.  Every thread calls.
__device__ __forceinline__ int block_excl_scan(int v, int *lds /*VOX_WAVES*/, int *total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < VOX_WAVES; ++k) {
        const int s = lds[k];
        if (k < w) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// V1, insert.  grid (blocks of rows, B).
__global__ __launch_bounds__(VOX_THREADS) void vox_insert_kernel(
    const float *__restrict__ points, int M, int cols, int dim, float inv, float pad_val, int cap,
    unsigned long long *__restrict__ keys, int32_t *__restrict__ slot_min, int32_t *__restrict__ slot_cnt,
    int32_t *__restrict__ row_slot, unsigned *__restrict__ pmax)
{
    const int b = blockIdx.y, i = blockIdx.x * VOX_THREADS + threadIdx.x;
    bool valid = i < M;
    unsigned mbits = 0u;
    unsigned long long key = 0ull;
    if (valid) {
        const float *row = points + ((size_t)b * M + i) * cols;
        unsigned long long mul = 1ull;
        for (int c = 0; c < cols; ++c) {
            const float x = row[c];
            const unsigned a = __float_as_uint(x) & 0x7fffffffu;
            valid = valid && a < 0x7f800000u;
            mbits = max(mbits, a);
            if (c < dim) {
                valid = valid && fabsf(x) < pad_val;
                const int cell = (int)floorf(x * inv);                     // one fp32 product and a floor: no division here
                key += (unsigned long long)((long long)cell + VOX_HALF) * mul;      // (a padding row's key is never used)
                mul *= VOX_SPAN;
            }
        }
    }
    // the pair's max|value| over the valid rows: one atomic per wave
    unsigned wmax = valid ? mbits : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) wmax = max(wmax, (unsigned)__shfl_xor((int)wmax, off, 64));
    if ((threadIdx.x & 63) == 0 && wmax != 0u) atomicMax(&pmax[b], wmax);
    if (i >= M) return;
    int slot = -1;
    if (valid) {
        unsigned long long h = key;
        h ^= h >> 33;
        h *= 0xff51afd7ed558ccdull;
        h ^= h >> 33;
        h *= 0xc4ceb9fe1a85ec53ull;
        h ^= h >> 33;
        unsigned long long *kb = keys + (size_t)b * cap;
        int s = (int)(h & (unsigned long long)(cap - 1));
        for (int step = 0; step < cap; ++step) {                           // bounded: at most M <= cap / 2 slots are ever taken
            const unsigned long long prev = atomicCAS(&kb[s], VOX_EMPTY, key);
            if (prev == VOX_EMPTY || prev == key) {
                slot = s;
                break;
            }
            s = (s + 1) & (cap - 1);
        }
        if (slot >= 0) {
            atomicMin(&slot_min[(size_t)b * cap + slot], i);
            atomicAdd(&slot_cnt[(size_t)b * cap + slot], 1);
        }
    }
    row_slot[(size_t)b * M + i] = slot;
}

__device__ __forceinline__ bool vox_leads(const int32_t *__restrict__ row_slot, const int32_t *__restrict__ slot_min, int b, int M,
                                          int cap, int i, int *slot_out)
{
    int slot = -1;
    if (i < M) slot = row_slot[(size_t)b * M + i];
    *slot_out = slot;
    return slot >= 0 && slot_min[(size_t)b * cap + slot] == i;
}

// V1, leaders (1): leaders per block of rows.  grid (blocks of rows, B).
__global__ __launch_bounds__(VOX_THREADS) void vox_count_kernel(const int32_t *__restrict__ row_slot,
                                                                 const int32_t *__restrict__ slot_min, int M, int cap,
                                                                 int32_t *__restrict__ blk)
{
    __shared__ int lds[VOX_WAVES];
    const int b = blockIdx.y, i = blockIdx.x * VOX_THREADS + threadIdx.x;
    int slot, total;
    const bool lead = vox_leads(row_slot, slot_min, b, M, cap, i, &slot);
    block_excl_scan(lead ? 1 : 0, lds, &total);
    if (threadIdx.x == 0) blk[(size_t)b * gridDim.x + blockIdx.x] = total;
}

// V1, leaders (2): the block counts of a pair -> their exclusive prefix sums (in place) and the pair's count.  grid (B).
__global__ __launch_bounds__(VOX_THREADS) void vox_scan_kernel(int32_t *__restrict__ blk, int nblk, int32_t *__restrict__ out_count)
{
    __shared__ int lds[VOX_WAVES];
    const int b = blockIdx.x;
    int32_t *pb = blk + (size_t)b * nblk;
    int carry = 0;
    for (int base = 0; base < nblk; base += VOX_THREADS) {
        const int j = base + threadIdx.x;
        const int v = j < nblk ? pb[j] : 0;
        int total;
        const int excl = block_excl_scan(v, lds, &total);
        if (j < nblk) pb[j] = carry + excl;
        carry += total;
    }
    if (threadIdx.x == 0) out_count[b] = carry;
}

// V1, leaders (3): the rank of every leader's slot, and the slot of every kept rank.  grid (blocks of rows, B).
__global__ __launch_bounds__(VOX_THREADS) void vox_rank_kernel(const int32_t *__restrict__ row_slot,
                                                                const int32_t *__restrict__ slot_min,
                                                                const int32_t *__restrict__ blk, int M, int cap, int max_out,
                                                                int32_t *__restrict__ slot_rank, int32_t *__restrict__ rank_slot)
{
    __shared__ int lds[VOX_WAVES];
    const int b = blockIdx.y, i = blockIdx.x * VOX_THREADS + threadIdx.x;
    int slot, total;
    const bool lead = vox_leads(row_slot, slot_min, b, M, cap, i, &slot);
    const int excl = block_excl_scan(lead ? 1 : 0, lds, &total);
    if (!lead) return;
    const int rank = blk[(size_t)b * gridDim.x + blockIdx.x] + excl;
    slot_rank[(size_t)b * cap + slot] = rank;
    if (rank < max_out) rank_slot[(size_t)b * max_out + rank] = slot;
}

// V1, accumulate.  One thread per (row, lane), L = 1 << lshift >= cols lanes per row, so that an atomic wave-instruction
// adds 64 / L whole rows (the shape of icp_bwd_target_scatter_kernel); a wave whose kept rows all share one cell sums them
// first and adds once per column.  CENTROID = false only writes voxel_of.  grid (blocks of (row, lane), B).
template <bool CENTROID>
__global__ __launch_bounds__(VOX_THREADS) void vox_accumulate_kernel(
    const float *__restrict__ points, const int32_t *__restrict__ row_slot, const int32_t *__restrict__ slot_rank,
    const unsigned *__restrict__ pmax, int M, int cols, int lshift, int cap, int max_out, int cnt_bits,
    unsigned long long *__restrict__ acc, int32_t *__restrict__ voxel_of)
{
    const int L = 1 << lshift, b = blockIdx.y;
    const long long t = (long long)blockIdx.x * VOX_THREADS + threadIdx.x;
    const long long i = t >> lshift;
    const int c = (int)(t & (L - 1));
    int rank = -1;
    if (i < M) {
        const int slot = row_slot[(size_t)b * M + i];
        if (slot >= 0) rank = slot_rank[(size_t)b * cap + slot];
        if (c == 0 && voxel_of != nullptr) voxel_of[(size_t)b * M + i] = rank;
    }
    if constexpr (CENTROID) {
        const bool kept = rank >= 0 && rank < max_out;
        long long v = 0;
        if (kept && c < cols) v = llrint((double)points[((size_t)b * M + i) * cols + c] * tgt_fixed_scale(pmax[b], cnt_bits));
        const unsigned long long kmask = __ballot(kept);
        if (kmask == 0ull) return;                                          // (uniform over the wave)
        unsigned long long *ab = acc + (size_t)b * max_out * L;
        const int r0 = __shfl(rank, __ffsll(kmask) - 1, 64);
        if (__ballot(kept && rank != r0) == 0ull) {
            for (int off = 32; off >= L; off >>= 1) v += __shfl_xor(v, off, 64);
            if ((threadIdx.x & 63) < L && v != 0) atomicAdd(&ab[(size_t)r0 * L + c], (unsigned long long)v);
        } else if (v != 0) {
            atomicAdd(&ab[(size_t)rank * L + c], (unsigned long long)v);
        }
    }
}

// V1, finalise.  One thread per output row.  grid (blocks of output rows, B).
template <bool CENTROID>
__global__ __launch_bounds__(VOX_THREADS) void vox_finalise_kernel(
    const float *__restrict__ points, const unsigned long long *__restrict__ acc, const unsigned *__restrict__ pmax,
    const int32_t *__restrict__ rank_slot, const int32_t *__restrict__ slot_min, const int32_t *__restrict__ slot_cnt,
    const int32_t *__restrict__ out_count, int M, int cols, int L, int cap, int max_out, int cnt_bits, int normals, float pad_val,
    float *__restrict__ out, int32_t *__restrict__ out_n, int32_t *__restrict__ out_first)
{
    const int b = blockIdx.y, r = blockIdx.x * VOX_THREADS + threadIdx.x;
    if (r >= max_out) return;
    float *o = out + ((size_t)b * max_out + r) * cols;
    int n = 0, first = -1;
    if (r < min(out_count[b], max_out)) {
        const int slot = rank_slot[(size_t)b * max_out + r];
        n = slot_cnt[(size_t)b * cap + slot];
        first = slot_min[(size_t)b * cap + slot];
        if constexpr (CENTROID) {
            const double scale = tgt_fixed_scale(pmax[b], cnt_bits);
            const unsigned long long *a = acc + ((size_t)b * max_out + r) * L;
            double len = 1.0;
            if (normals) {
                const double nx = (double)(long long)a[3] / scale / n, ny = (double)(long long)a[4] / scale / n,
                             nz = (double)(long long)a[5] / scale / n;
                len = sqrt(nx * nx + ny * ny + nz * nz);
            }
            for (int c = 0; c < cols; ++c) {
                double m = (double)(long long)a[c] / scale / n;
                if (normals && c >= 3 && c < 6) m = len == 0.0 ? 0.0 : m / len;
                o[c] = (float)m;
            }
        } else {
            const float *row = points + ((size_t)b * M + first) * cols;
            for (int c = 0; c < cols; ++c) o[c] = row[c];
        }
    } else {
        for (int c = 0; c < cols; ++c) o[c] = pad_val;
    }
    if (out_n != nullptr) out_n[(size_t)b * max_out + r] = n;
    if (out_first != nullptr) out_first[(size_t)b * max_out + r] = first;
}

struct VoxWs {
    unsigned long long *keys, *acc;
    int32_t *slot_min, *slot_cnt, *slot_rank, *row_slot, *rank_slot, *blk;
    unsigned *pmax;
    size_t zero_bytes, bytes;        // zero_bytes: slot_cnt .. pmax, one memset
};

VoxWs vox_carve(int32_t B, int32_t M, int32_t cols, int32_t max_out, void *workspace, size_t workspace_bytes)
{
    mmk::Arena ar(workspace, workspace_bytes);
    const size_t cap = (size_t)vox_cap(M);
    VoxWs w;
    w.keys = ar.take<unsigned long long>((size_t)B * cap);
    w.slot_min = ar.take<int32_t>((size_t)B * cap);
    w.slot_cnt = ar.take<int32_t>((size_t)B * cap);
    w.acc = ar.take<unsigned long long>((size_t)B * max_out * vox_lanes(cols));
    w.pmax = ar.take<unsigned>((size_t)B);
    w.zero_bytes = (size_t)((char *)(w.pmax + B) - (char *)w.slot_cnt);
    w.slot_rank = ar.take<int32_t>((size_t)B * cap);
    w.row_slot = ar.take<int32_t>((size_t)B * M);
    w.rank_slot = ar.take<int32_t>((size_t)B * max_out);
    w.blk = ar.take<int32_t>((size_t)B * vox_blocks(M));
    w.bytes = mmk::align_up(ar.off, 256);
    return w;
}

bool vox_sizes_ok(int32_t B, int32_t M, int32_t cols, int32_t max_out)
{
    return B >= 1 && B <= 65535 && M >= 1 && M <= VOX_MAX_M && cols >= 2 && cols <= 8 && max_out >= 1;
}

}  // namespace

extern "C" size_t mmk_voxel_downsample_workspace_bytes(int32_t B, int32_t M, int32_t cols, int32_t max_out)
{
    if (!vox_sizes_ok(B, M, cols, max_out)) return 0;
    return vox_carve(B, M, cols, max_out, nullptr, 0).bytes;
}

extern "C" int mmk_voxel_downsample(const float *points, int32_t B, int32_t M, int32_t cols, int32_t dim, float voxel, float pad_val,
                                    int32_t mode, int32_t normals, int32_t max_out, float *out, int32_t *out_count, int32_t *out_n,
                                    int32_t *out_first, int32_t *voxel_of, void *workspace, size_t workspace_bytes, void *stream)
{
    MMK_REQUIRE(points && out && out_count, "mmk_voxel_downsample: NULL pointer (points, out and out_count are required)");
    MMK_REQUIRE(B >= 1 && B <= 65535, "mmk_voxel_downsample: B must be in 1..65535 (got %d)", B);
    MMK_REQUIRE(M >= 1 && M <= VOX_MAX_M, "mmk_voxel_downsample: M must be in 1..2^28 (got %d)", M);
    MMK_REQUIRE(dim == 2 || dim == 3, "mmk_voxel_downsample: dim must be 2|3 (got %d)", dim);
    MMK_REQUIRE(cols >= dim && cols <= 8, "mmk_voxel_downsample: cols must be in dim..8 (got %d, dim %d)", cols, dim);
    MMK_REQUIRE(isfinite(voxel) && voxel > 0.f, "mmk_voxel_downsample: voxel must be finite and > 0 (got %g)", (double)voxel);
    MMK_REQUIRE(isfinite(pad_val) && pad_val > 0.f, "mmk_voxel_downsample: pad_val must be finite and > 0 (got %g)", (double)pad_val);
    const float inv = (float)(1.0 / (double)voxel);
    const float reach = pad_val * inv;
    MMK_REQUIRE(reach <= 1048576.f, "mmk_voxel_downsample: pad_val / voxel must be <= 2^20 cells (got %g)", (double)reach);
    MMK_REQUIRE(mode == MMK_VOXEL_CENTROID || mode == MMK_VOXEL_FIRST, "mmk_voxel_downsample: unknown mode %d", mode);
    MMK_REQUIRE(normals == 0 || normals == 1, "mmk_voxel_downsample: normals must be 0|1 (got %d)", normals);
    MMK_REQUIRE(normals == 0 || cols >= 6, "mmk_voxel_downsample: normals = 1 needs cols >= 6 (got %d)", cols);
    MMK_REQUIRE(max_out >= 1, "mmk_voxel_downsample: max_out must be >= 1 (got %d)", max_out);
    const VoxWs w = vox_carve(B, M, cols, max_out, workspace, workspace_bytes);
    MMK_REQUIRE(workspace != nullptr && w.bytes <= workspace_bytes, "mmk_voxel_downsample: workspace too small (%zu < %zu bytes)",
                workspace ? workspace_bytes : (size_t)0, w.bytes);
    hipStream_t st = (hipStream_t)stream;
    const int cap = vox_cap(M), nblk = vox_blocks(M), L = vox_lanes(cols);
    int lshift = 0, cnt_bits = 0;
    while ((1 << lshift) < L) ++lshift;
    while (((size_t)1 << cnt_bits) < (size_t)M) ++cnt_bits;
    MMK_CHECK_HIP(hipMemsetAsync(w.keys, 0xFF, sizeof(unsigned long long) * (size_t)B * cap, st));
    MMK_CHECK_HIP(hipMemsetAsync(w.slot_min, 0x7F, sizeof(int32_t) * (size_t)B * cap, st));         // 0x7f7f7f7f > every row index
    MMK_CHECK_HIP(hipMemsetAsync(w.slot_cnt, 0, w.zero_bytes, st));
    const dim3 rows(nblk, B), threads(VOX_THREADS);
    hipLaunchKernelGGL(vox_insert_kernel, rows, threads, 0, st, points, M, cols, dim, inv, pad_val, cap, w.keys, w.slot_min, w.slot_cnt,
                       w.row_slot, w.pmax);
    MMK_LAUNCH_CHECK();
    hipLaunchKernelGGL(vox_count_kernel, rows, threads, 0, st, w.row_slot, w.slot_min, M, cap, w.blk);
    MMK_LAUNCH_CHECK();
    hipLaunchKernelGGL(vox_scan_kernel, dim3(B), threads, 0, st, w.blk, nblk, out_count);
    MMK_LAUNCH_CHECK();
    hipLaunchKernelGGL(vox_rank_kernel, rows, threads, 0, st, w.row_slot, w.slot_min, w.blk, M, cap, max_out, w.slot_rank, w.rank_slot);
    MMK_LAUNCH_CHECK();
    const dim3 lanes((unsigned)(((size_t)M * L + VOX_THREADS - 1) / VOX_THREADS), B), outs((max_out + VOX_THREADS - 1) / VOX_THREADS, B);
    if (mode == MMK_VOXEL_CENTROID) {
        hipLaunchKernelGGL(vox_accumulate_kernel<true>, lanes, threads, 0, st, points, w.row_slot, w.slot_rank, w.pmax, M, cols, lshift, cap,
                           max_out, cnt_bits, w.acc, voxel_of);
        MMK_LAUNCH_CHECK();
        hipLaunchKernelGGL(vox_finalise_kernel<true>, outs, threads, 0, st, points, w.acc, w.pmax, w.rank_slot, w.slot_min, w.slot_cnt,
                           out_count, M, cols, L, cap, max_out, cnt_bits, normals, pad_val, out, out_n, out_first);
    } else {
        if (voxel_of != nullptr) {                    // one lane per row: nothing is summed
            hipLaunchKernelGGL(vox_accumulate_kernel<false>, rows, threads, 0, st, points, w.row_slot, w.slot_rank, w.pmax, M, cols, 0,
                               cap, max_out, cnt_bits, w.acc, voxel_of);
            MMK_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(vox_finalise_kernel<false>, outs, threads, 0, st, points, w.acc, w.pmax, w.rank_slot, w.slot_min, w.slot_cnt,
                           out_count, M, cols, L, cap, max_out, cnt_bits, normals, pad_val, out, out_n, out_first);
    }
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}
