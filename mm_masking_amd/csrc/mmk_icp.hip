// Differentiable ICP on gfx950: brute-force nearest neighbour (LDS-tiled), robust
// weighted normal-equation accumulation (wave64 shuffle reduction), 3x3 / 6x6
// Gauss-Newton solve + SE(2)/SE(3) exponential update, and the reverse sweep.
//
// Replaces dICP.ICP.ICP(...).icp(...) as called from the reference at
// mm_masking/icp_weight_policy.py:281-287 (external/dICP itself is absent from the
// reference tree).  The arithmetic is the normative spec of DESIGN.md §3 and is
// restated on the CPU in oracle/dicp_ref.py + oracle/nn_search.c; per-point fp32
// operations are written in the same order as there and this file MUST be built
// with -ffp-contract=off so that only the explicit fmaf calls fuse.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "mmk_common.h"

namespace {

constexpr int NN_THREADS = 256;
constexpr int NN_TILE = 1024;  // target points staged in LDS per tile
constexpr float NN_PAD = 3.0e18f;
constexpr int ACC_THREADS = 256;
constexpr int PART_ROWS = 32;         // rows of block partials staged in LDS per round by the per-pair kernels

__host__ __device__ constexpr int nacc(int dim) { return dim == 2 ? 9 : 27; }
__host__ __device__ constexpr int npose(int dim) { return dim == 2 ? 6 : 12; }

// ------------------------------------------------------------------------------------------
// I1: p = R s + t, fp32, individually rounded left to right (oracle: transform_points).
template <int DIM>
__device__ __forceinline__ void transform_point(const float *T, const float s[3], float p[DIM])
{
    if constexpr (DIM == 2) {
        p[0] = (T[0] * s[0] + T[1] * s[1]) + T[3];
        p[1] = (T[4] * s[0] + T[5] * s[1]) + T[7];
    } else {
        p[0] = ((T[0] * s[0] + T[1] * s[1]) + T[2] * s[2]) + T[3];
        p[1] = ((T[4] * s[0] + T[5] * s[1]) + T[6] * s[2]) + T[7];
        p[2] = ((T[8] * s[0] + T[9] * s[1]) + T[10] * s[2]) + T[11];
    }
}

// Squared distance in the fmaf form of oracle/nn_search.c.
template <int DIM>
__device__ __forceinline__ float nn_dist(float tx, float ty, float tz, const float p[DIM])
{
    float dx = tx - p[0];
    float dy = ty - p[1];
    float d = __builtin_fmaf(dy, dy, dx * dx);
    if constexpr (DIM == 3) {
        float dz = tz - p[2];
        d = __builtin_fmaf(dz, dz, d);
    }
    return d;
}

// ------------------------------------------------------------------------------------------
// Planar, padded copy of the target coordinates: (B,M,cols) AoS -> (B,DIM,Mpad).
// `dec` (optional, (B, dim, Mpad / dec_stride)): every dec_stride-th target again, densely -- the samples of the first
// iteration's coarse seed pass (nn_coarse_seed_kernel), which would otherwise gather them 4 bytes at a time.
__global__ void pack_target_kernel(const float *__restrict__ tgt, int M, int cols, int dim, int Mpad,
                                   float *__restrict__ out, float *__restrict__ dec, int dec_stride)
{
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    int b = blockIdx.y;
    if (j >= Mpad) return;
    for (int c = 0; c < dim; ++c) {
        float v = NN_PAD;
        if (j < M) v = tgt[((size_t)b * M + j) * cols + c];
        out[((size_t)b * dim + c) * Mpad + j] = v;
        if (dec != nullptr && j % dec_stride == 0) dec[((size_t)b * dim + c) * (Mpad / dec_stride) + j / dec_stride] = v;
    }
}

// ------------------------------------------------------------------------------------------
// I2: brute-force NN with an exact pre-filter.  The derivation below is the vector-pipe form of rounds 2-3 (kernel removed in
// round 5: HISTORY.md 5, 9.1); the kernel of this file prices the pairs on the matrix cores (nn_mfma_kernel, further down) with
// the same unit decomposition, seeds and exact re-scan.  Work is cut into units (pair, source block, target range); a persistent 1-D grid walks them with
// stride gridDim.x.  Units are numbered so that unit % 8 == pair % 8: blocks of one pair share an XCD (blockIdx % 8 label) and
// its target planes stay in that L2.  The partial results of the target ranges meet in one 64-bit atomic min per source point
// on the key (float bits of d2) << 32 | index: d2 >= 0, so unsigned order == float order, and equal distances resolve to the
// lowest index; min is order independent, so the result is deterministic.
// A plain scan spends 4.5 vector lane-operations per (point, target) pair on d = fma(dy, dy, dx * dx) (round 1's kernel:
// bound by the fp32 VALU).  Here every pair is first priced with the expanded form
//      e_j = fma(tx_j, a, fma(ty_j, b, tn_j)),   a = -2 px, b = -2 py,  tn_j = |t_j|^2 (formed once per target while
//      its tile is staged into LDS)              -> 2 lane-operations (+ 1/2 for the running minimum)
// which equals D_j - |p|^2 up to rounding, D_j the true squared distance.  Still exhaustive: every target is
// visited by every point; only targets that can be the argmin are evaluated with the normative formula.
//
// Exactness.  u = 2^-24.  The normative value obeys |d_j - D_j| <= 5u D_j (four relative roundings).  For a
// target with |t_j| <= |p| + sqrt(D_j):  |e_j - (D_j - |p|^2)| <= G(D_j), G(D) = u (7.1 |p|^2 + 10.1 |p| sqrt(D) +
// 5.1 D)  [tn: 2 roundings; each fma one rounding of a partial sum bounded by |t|^2 + 2 |p||t|].  Let j* be the
// normative argmin and m the argmin of e, X = D_m.  d_j* <= d_k for all k gives D_j* <= X (1 + 11u), hence
//      e_j* - e_m <= 11u X + G(X (1 + 11u)) + G(X) <= u (24.3 |p|^2 + 31.4 X),   X <= (e_m + |p|^2)(1 + 13u).
// So j* lies among the targets with e_j <= thr(e_m), thr(b) = b + kappa (|p|^2 + max(0, b + |p|^2)), kappa = 48u
// (dim 2; 64u for dim 3 where the same derivation gives u (38 |p|^2 + 41 X)): the constants leave > 30 % of slack
// for the fp32 evaluation of thr itself.  thr is monotone in b, so testing a chunk of 32 targets against the
// RUNNING minimum b_run >= e_m flags a superset of the chunks that hold such a target; the flagged chunks (one
// bit each) are then re-scanned with nn_dist() -- from the LDS tile, before the next tile is staged -- in ascending
// order with a strict '<', which yields exactly the lowest-index argmin of the oracle (oracle/nn_search.c):
// tests/test_gpu_icp.py::test_nn_bit_exact.  b_run starts from e of the previous iteration's correspondent (any
// e_j bounds the minimum), so after the first iteration little more than the chunks that matter is flagged.
constexpr int PF_CH = 32;            // targets per flag bit (32 chunks per LDS tile: one flag word per point and tile)

// Identical source rows have identical nearest neighbours.  The reference pads every scan with all-zero rows up to the
// largest cloud of the data set (icp_weight_dataset.py:377-381: about half of the 5 120 rows of a synthetic scan), and all
// of them map to the same transformed point.  Once per icp() call this kernel finds, per pair, the first all-zero row
// (zrep) and the source blocks that hold nothing else (allzero); a block that is all zero and lies behind zrep is not
// scanned at all -- its rows take the key of row zrep, which an earlier block computed (icp_accumulate_kernel) --
// exactly what the scan would have returned for them.
__global__ __launch_bounds__(NN_THREADS) void src_zero_scan_kernel(const float *__restrict__ src, int N, int pts, int nsb,
                                                                  int32_t *__restrict__ allzero, int32_t *__restrict__ zrep)
{
    const int sb = blockIdx.x, b = blockIdx.y;
    int first = N;
    int nonzero = 0;
    for (int q = threadIdx.x; q < pts; q += blockDim.x) {
        const int i = sb * pts + q;
        if (i < N) {
            const float *sp = src + ((size_t)b * N + i) * 3;
            const bool z = sp[0] == 0.f && sp[1] == 0.f && sp[2] == 0.f;
            nonzero |= z ? 0 : 1;
            if (z && i < first) first = i;
        }
    }
    const int any = __syncthreads_or(nonzero);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) first = min(first, __shfl_down(first, off, 64));
    if ((threadIdx.x & 63) == 0 && first < N) atomicMin(&zrep[b], first);
    if (threadIdx.x == 0) allzero[(size_t)b * nsb + sb] = any ? 0 : 1;
}

// The source blocks that are scanned, as dense lists: one list per class b % 8 (the class picks the XCD whose L2 holds the
// pair's target, as in the kernels' unit numbering), entries (b << 12 | sb) in ascending (b, sb); ucnt[c] = length of
// list c, ucnt[8] = the longest.  With the skipped blocks gone from the numbering the persistent blocks of the NN kernel
// all get the same amount of work (with `continue` on a skipped unit some blocks had two units and others none).
__global__ void src_units_kernel(const int32_t *__restrict__ allzero, const int32_t *__restrict__ zrep, int B, int nsb, int pts,
                                 int cap, int32_t *__restrict__ ulist, int32_t *__restrict__ ucnt)
{
    const int c = threadIdx.x;
    int n = 0;
    if (c < 8)
        for (int b = c; b < B; b += 8)
            for (int sb = 0; sb < nsb; ++sb)
                if (!(allzero[(size_t)b * nsb + sb] != 0 && zrep[b] < sb * pts)) ulist[(size_t)c * cap + n++] = (b << 12) | sb;
    if (c < 8) ucnt[c] = n;
    int mx = n;
#pragma unroll
    for (int off = 4; off > 0; off >>= 1) mx = max(mx, __shfl_down(mx, off, 64));
    if (c == 0) ucnt[8] = mx;
}

// ------------------------------------------------------------------------------------------
// I2, the brute-force engine: the exact pre-filter above with every (point, target) pair priced on the MATRIX cores.  The fp32 VALU is what bounds the scan above (2 FMAs + 1/2 min per pair); the
// bf16 matrix pipe runs beside the vector pipe and prices 32 x 32 pairs per v_mfma_f32_32x32x16_bf16 (32 cycles per SIMD),
// which leaves the vector pipe the chunk minima and the flags only: ~0.8 vector instructions per 64 pairs instead of 3.3.
//
// How a bf16 product gives an fp32-grade filter.  An fp32 number splits EXACTLY into three bf16 pieces, x = x1 + x2 + x3
// (x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2): 8 + 8 + 8 significant bits, |x2| <= 2^-9 |x|, |x3| <= 2^-18 |x|),
// products of pieces are exact in fp32, and the matrix core accumulates in fp32.  With a = -2p (exact) and n = fl(|t|^2)
// (formed in fp32 while the tile is staged: |n - |t|^2| <= 2u |t|^2, u = 2^-24), the 16 k-slots of one instruction hold
//      k0..5   tx1 ax1, tx2 ax1, tx1 ax2, tx3 ax1, tx2 ax2, tx1 ax3        (= tx ax up to 2^-26 |tx ax|: the three
//      k6..11  ty1 ay1, ty2 ay1, ty1 ay2, ty3 ay1, ty2 ay2, ty1 ay3         products left out are <= 2^-27, 2^-27, 2^-36)
//      k12..14 n1 * 1, n2 * 1, n3 * 1;  k15 = 0
// so that E_j = sum_k A[j][k] B[k][i] equals e_j = |t_j|^2 - 2 p_i . t_j = D_j - |p|^2 up to
//      |E_j - e_j| <= 2u |t|^2 + u/2 |t||p| + 32.7u (|t|^2 + 2 |t||p|)
// -- the last term for the accumulation of the <= 16 addends in WHATEVER order the hardware adds them, each addition charged
// 2u of the sum of magnitudes S <= 1.02 (|t|^2 + 2|t||p|) (twice the rounding unit: also covers truncating adders).  With
// |t| <= |p| + sqrt(D) and 2 |p| sqrt(D) <= |p|^2 + D:   |E_j - e_j| <= G(D_j),  G(D) = u (168.3 |p|^2 + 102.4 D).
// The fp32 seed of the running bound (e of the previous iteration's correspondent, the fma chain e = fma(tx, a, fma(ty, b, tn)))
// errs by less than that.  Exactness then follows as above: j* the normative argmin, m the target whose computed value is
// the running bound b, X = D_m: D_j* <= X (1 + 11u), so
//      E_j* <= e_m + 11u X + G(X (1 + 11u)) <= b + G(X) + 11u X + G(X(1 + 11u)) <= b + u (336.6 |p|^2 + 216 X),
//      X <= (b + |p|^2)(1 + 103u) + 169u |p|^2,
// i.e. j* lies in a chunk whose minimum is <= thr(b), thr(b) = b + kappa (|p|^2 + (b + |p|^2)) = b (1 + kappa) + 2 kappa |p|^2,
// kappa = 352u (15u |p|^2 of slack for the fp32 evaluation of thr; b + |p|^2 < 0 happens by rounding only, where X is
// O(u |p|^2) and the term it multiplies is immaterial).  The kernel tests min < thr with kappa = 360u (strict: the chain of
// v_min3 starts from thr itself), which flags whatever min <= thr flags at 352u: thr_360 - thr_352 = 8u (|p|^2 + D) > 0,
// and c2 carries an absolute 1e-30 for the point that sits on the origin.  thr is monotone in b, every lane tests the 16 values it holds of a
// 32-target chunk against ITS OWN running minimum (an upper bound of the true one: a superset of the chunks is flagged), the
// two lanes that share a point OR their flag words, and the flagged chunks are re-scanned with nn_dist() from the fp32
// planes kept in LDS next to the fragments -- ascending, strict '<': exactly the oracle's lowest-index argmin, as before
// (tests/test_gpu_icp.py::test_nn_bit_exact and every ICP test; kappa is 7x the VALU filter's, which costs re-scans --
// 0.03 m^2 of margin at 35 m from the sensor -- not correctness).
// Layout: a block of 4 waves takes a source block of 512 points (the unit decomposition, XCD classes, zero-row lists and
// 64-bit atomic-min merge are those of the kernels above); wave w holds 4 groups of 32 points as B operands (columns);
// a tile of 1 024 targets sits in LDS as 32 A fragments [chunk][lane][8 bf16] (lane l: target l & 31, k = 8 (l >> 5) ...),
// written by the thread that staged the target; the result tile has the point on the lane (column l & 31) and 16 targets
// in the lane's registers.  For the re-scan and the output lane l owns the points of groups 2 (l >> 5) + {0, 1}.
typedef __attribute__((ext_vector_type(8))) __bf16 nn_bf16x8;
typedef __attribute__((ext_vector_type(16))) float nn_f32x16;
constexpr int NNM_GROUPS = 4;                      // 32-point groups per wave
constexpr int NNM_PTS = NN_THREADS / 64 * NNM_GROUPS * 32;    // 512 points per block

// D = A B (C = 0).  The compiler builtin, NOT inline asm: hipcc then keeps the result tile in VGPRs (gfx950's register file is
// unified; the vector pipe consumes the tile at once) and pads the MFMA -> VALU read hazard itself (s_nop 8-10 behind each pair
// of MFMAs; nothing is padded around asm statements).  Measured equal to a hand-scheduled asm form (134 us per launch either way).
__device__ __forceinline__ nn_f32x16 mfma_32x32x16_bf16_c0(nn_bf16x8 a, nn_bf16x8 b)
{
    const nn_f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, z, 0, 0, 0);
}
__device__ __forceinline__ void split3(float x, __bf16 &x1, __bf16 &x2, __bf16 &x3)
{
    x1 = (__bf16)x;
    const float r = x - (float)x1;
    x2 = (__bf16)r;
    x3 = (__bf16)(r - (float)x2);
}

// dim 3 (round 4): 21 k-slots -- 6 products per coordinate and the three pieces of |t|^2 -- fill two k-slices, i.e. two chained
// MFMAs per (32 targets x 32 points); the target tile is staged 512 targets at a time so that the fragments still take 32 KB
// (four blocks per CU by LDS; three by registers).  Error bound, same derivation with three coordinates: n = fl(|t|^2) carries
// three roundings (3u |t|^2), the nine dropped products u/2 |t||p| (Cauchy-Schwarz over the coordinates), the 21 addends and the
// chaining addition are charged 2u S each, S <= 1.02 (|t|^2 + 2 |t||p|): |E_j - e_j| <= 48u |t|^2 + 90.5u |t||p| <= G3(D) =
// u (231.8 |p|^2 + 141.3 D).  The normative distance has one more fma: |d - D| <= 6u D, D_j* <= X (1 + 13u).  Hence
// E_j* <= b + u (463.5 |p|^2 + 296 X), X <= (b + |p|^2)(1 + 145u) + 232u |p|^2, and thr(b) = b (1 + kappa) + 2 kappa |p|^2 with
// kappa = 496u covers it with 15u |p|^2 to spare for its own evaluation (launch_nn passes 496u for dim 3, 360u for dim 2).
template <int DIM>
__global__ __launch_bounds__(NN_THREADS, DIM == 2 ? 4 : 3) void nn_mfma_kernel(
    const float *__restrict__ src, const float *__restrict__ tgtp,
    const float *__restrict__ Tk, const int32_t *__restrict__ active, const int32_t *__restrict__ prev_idx,
    const int32_t *__restrict__ ulist, const int32_t *__restrict__ ucnt, int ucap, int B,
    int N, int Mpad, int nsb, int ntu, int tiles_per_unit, int total_units, float kappa,
    unsigned long long *__restrict__ packed)
{
    static_assert((DIM == 2 || DIM == 3) && NNM_GROUPS == 4, "the matrix-core filter: 16 (dim 2) or 2 x 16 (dim 3) k-slots, 4 point groups per wave");
    constexpr int KS = DIM == 2 ? 1 : 2;             // k-slices = chained MFMAs per chunk
    constexpr int TT = NN_TILE / KS;                 // targets staged per sub-tile
    constexpr int NCH = TT / 32;                     // chunks per sub-tile (one flag bit each)
    constexpr int TPT = TT / NN_THREADS;             // targets a thread stages: 4 (dim 2) or 2 (dim 3)
    __shared__ __attribute__((aligned(16))) uint4 frag[KS][NCH][64];             // 32 KB: A fragments of the sub-tile
    // the fp32 planes (exact re-scan), 8 / 6 KB, laid out plainly.  In the re-scan every lane reads the eight float4s of ITS OWN
    // flagged chunk, so chunks of one parity share eight 16-byte bank slots and 45 % of the kernel's LDS cycles are conflict
    // cycles (profiles/r03_nn_pmc_counters.json) -- which costs no time: a conflict-free image (float4 h of chunk c at position
    // h ^ ((c >> 1) & 7)) was measured 1-3 us per launch SLOWER (131-134 against 130-131 us: eight more vector instructions
    // per re-scanned chunk on a loop the vector pipe binds, round 4), so the plain image stays.
    __shared__ __attribute__((aligned(16))) float lt[DIM][TT];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int col = lane & 31, half = lane >> 5;
    const int ntiles = Mpad / NN_TILE;
    if (ulist != nullptr) total_units = ucnt[8] * ntu * 8;
    const float kp1 = 1.0f + kappa;

    // (static stride over the units, as in the kernels above.  A work queue -- one atomic draw per unit from a head per XCD
    // class, issued a unit ahead -- was tried and lost 25-50 us per launch: the block-wide hand-over of the drawn unit costs
    // more than the imbalance it removes.)
    for (int u = blockIdx.x; u < total_units; u += gridDim.x) {
        const int xcd = u & 7;
        int rest = u >> 3;
        const int tu = rest % ntu;
        rest /= ntu;
        int sb, b;
        if (ulist != nullptr) {
            if (rest >= ucnt[xcd]) continue;
            const int code = ulist[(size_t)xcd * ucap + rest];
            sb = code & 0xfff;
            b = code >> 12;
        } else {
            sb = rest % nsb;
            b = (rest / nsb) * 8 + xcd;
        }
        if (b >= B) continue;
        if (active != nullptr && active[b] == 0) continue;

        float T[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) T[i] = Tk[(size_t)b * 16 + i];
        const float *tb = tgtp + (size_t)b * DIM * Mpad;

        // ---- the wave's 4 x 32 points: this lane's column of every group (both lanes l, l + 32 of a column do the same)
        // Coordinates as separate scalars, selected with v_cndmask.  As an array p[g][c] handed to transform_point() and then
        // read as `half ? p[2 + q] : p[q]` they became a 48-byte scratch-memory array read back at a run-time offset; with that
        // build 16-lane groups of a wave now and then worked on wrong coordinates (correspondences that changed from run to
        // run; a NaN coordinate finds nothing, so keys that nobody armed).  The round trip is sound in isolation
        // (scripts/ubench/scratch_roundtrip.hip) and so is the code object (HISTORY.md section 10); what failed in the full
        // process is not established.  The library uses no scratch memory anywhere:
        // tests/test_code_objects.py::test_no_kernel_uses_scratch_memory.
        float px[NNM_GROUPS], py[NNM_GROUPS], pz[NNM_GROUPS], c2[NNM_GROUPS], brun[NNM_GROUPS], thr[NNM_GROUPS], dseed[NNM_GROUPS];
        int jseed[NNM_GROUPS];
        nn_bf16x8 bfr[KS][NNM_GROUPS];
        unsigned w[NNM_GROUPS];
#pragma unroll
        for (int g = 0; g < NNM_GROUPS; ++g) {
            const int i = sb * NNM_PTS + wv * (NNM_GROUPS * 32) + g * 32 + col;
            float s0 = 0.f, s1 = 0.f, s2 = 0.f;
            if (i < N) {
                const float *sp = src + ((size_t)b * N + i) * 3;
                s0 = sp[0];
                s1 = sp[1];
                s2 = sp[2];
            }
            const float s[3] = {s0, s1, s2};
            float tp[DIM];
            transform_point<DIM>(T, s, tp);
            px[g] = tp[0];
            py[g] = tp[1];
            pz[g] = DIM == 3 ? tp[DIM - 1] : 0.f;
            float pn = tp[0] * tp[0] + tp[1] * tp[1];
            if constexpr (DIM == 3) pn += tp[DIM - 1] * tp[DIM - 1];
            c2[g] = 2.0f * kappa * pn + 1e-30f;
            const float ax = -2.0f * tp[0], ay = -2.0f * tp[1], az = -2.0f * pz[g];
            __bf16 ax1, ax2, ax3, ay1, ay2, ay3;
            split3(ax, ax1, ax2, ax3);
            split3(ay, ay1, ay2, ay3);
            const __bf16 one = (__bf16)1.0f, zero = (__bf16)0.0f;
            const nn_bf16x8 lo = {ax1, ax1, ax2, ax1, ax2, ax3, ay1, ay1};
            if constexpr (DIM == 2) {
                const nn_bf16x8 hi = {ay2, ay1, ay2, ay3, one, one, one, zero};
                bfr[0][g] = half ? hi : lo;
            } else {
                __bf16 az1, az2, az3;
                split3(az, az1, az2, az3);
                const nn_bf16x8 hi = {ay2, ay1, ay2, ay3, az1, az1, az2, az1};
                const nn_bf16x8 lo1 = {az2, az3, one, one, one, zero, zero, zero};
                const nn_bf16x8 hi1 = {zero, zero, zero, zero, zero, zero, zero, zero};
                bfr[0][g] = half ? hi : lo;
                bfr[KS - 1][g] = half ? hi1 : lo1;
            }
            // any e_j bounds the minimum: start from the previous iteration's correspondent (fp32 chain of the filter above)
            float b0 = INFINITY;
            dseed[g] = INFINITY;
            jseed[g] = -1;
            if (prev_idx != nullptr && i < N) {
                const int j = prev_idx[(size_t)b * N + i];
                if (j >= 0 && j < Mpad) {
                    const float jx = tb[j], jy = tb[(size_t)Mpad + j];
                    float jz = 0.f;
                    float jn = __builtin_fmaf(jy, jy, jx * jx);
                    float e = 0.f;
                    if constexpr (DIM == 3) {
                        jz = tb[(size_t)2 * Mpad + j];
                        jn = __builtin_fmaf(jz, jz, jn);
                        e = __builtin_fmaf(jz, az, __builtin_fmaf(jy, ay, jn));
                    } else {
                        e = __builtin_fmaf(jy, ay, jn);
                    }
                    b0 = __builtin_fmaf(jx, ax, e);
                    b0 = (b0 == b0) ? b0 : INFINITY;
                    const float dj = nn_dist<DIM>(jx, jy, jz, tp);       // the normative distance to the seed target
                    dseed[g] = (dj == dj) ? dj : INFINITY;
                    jseed[g] = j;
                }
            }
            brun[g] = b0;
            thr[g] = __builtin_fmaf(b0, kp1, c2[g]);
        }
        // ---- the two points this lane owns for the exact part
        float pox[2], poy[2], poz[2], cur[2], dso[2];
        int pidx[2], jj[2], jso[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            pox[q] = half ? px[2 + q] : px[q];
            poy[q] = half ? py[2 + q] : py[q];
            poz[q] = half ? pz[2 + q] : pz[q];
            pidx[q] = sb * NNM_PTS + wv * (NNM_GROUPS * 32) + (2 * half + q) * 32 + col;
            cur[q] = INFINITY;
            dso[q] = half ? dseed[2 + q] : dseed[q];
            jso[q] = half ? jseed[2 + q] : jseed[q];
        }

        const int t0 = tu * tiles_per_unit;
        const int t1 = min(ntiles, t0 + tiles_per_unit);
        jj[0] = jj[1] = t0 * NN_TILE;

        for (int t = t0 * KS; t < t1 * KS; ++t) {          // sub-tiles of TT targets
            __syncthreads();
            {   // stage: this thread's TPT targets -> the fp32 planes and rows TPT (tid % (32 / TPT)) .. of fragment tid / (32 / TPT)
                float xs[TPT], ys[TPT], zs[TPT];
                const int ch = tid / (32 / TPT), p4 = (tid % (32 / TPT)) * TPT;      // chunk, first target inside the chunk
                const int lpos = ch * 32 + p4;
                if constexpr (TPT == 4) {
                    const float4 vx = *reinterpret_cast<const float4 *>(tb + (size_t)t * TT + tid * 4);
                    const float4 vy = *reinterpret_cast<const float4 *>(tb + (size_t)Mpad + (size_t)t * TT + tid * 4);
                    *reinterpret_cast<float4 *>(&lt[0][lpos]) = vx;
                    *reinterpret_cast<float4 *>(&lt[1][lpos]) = vy;
                    xs[0] = vx.x; xs[1] = vx.y; xs[2] = vx.z; xs[3] = vx.w;
                    ys[0] = vy.x; ys[1] = vy.y; ys[2] = vy.z; ys[3] = vy.w;
#pragma unroll
                    for (int r = 0; r < TPT; ++r) zs[r] = 0.f;
                } else {
                    const float2 vx = *reinterpret_cast<const float2 *>(tb + (size_t)t * TT + tid * 2);
                    const float2 vy = *reinterpret_cast<const float2 *>(tb + (size_t)Mpad + (size_t)t * TT + tid * 2);
                    const float2 vz = *reinterpret_cast<const float2 *>(tb + (size_t)(DIM - 1) * Mpad + (size_t)t * TT + tid * 2);
                    *reinterpret_cast<float2 *>(&lt[0][lpos]) = vx;
                    *reinterpret_cast<float2 *>(&lt[1][lpos]) = vy;
                    *reinterpret_cast<float2 *>(&lt[DIM - 1][lpos]) = vz;
                    xs[0] = vx.x; xs[TPT - 1] = vx.y;
                    ys[0] = vy.x; ys[TPT - 1] = vy.y;
                    zs[0] = vz.x; zs[TPT - 1] = vz.y;
                }
                uint4 *fr = &frag[0][ch][p4];
#pragma unroll
                for (int r = 0; r < TPT; ++r) {
                    float n = __builtin_fmaf(ys[r], ys[r], xs[r] * xs[r]);
                    if constexpr (DIM == 3) n = __builtin_fmaf(zs[r], zs[r], n);
                    __bf16 x1, x2, x3, y1, y2, y3, n1, n2, n3;
                    split3(xs[r], x1, x2, x3);
                    split3(ys[r], y1, y2, y3);
                    split3(n, n1, n2, n3);
                    const nn_bf16x8 lo = {x1, x2, x1, x3, x2, x1, y1, y2};
                    fr[r] = __builtin_bit_cast(uint4, lo);
                    if constexpr (DIM == 2) {
                        const nn_bf16x8 hi = {y1, y3, y2, y1, n1, n2, n3, (__bf16)0.0f};
                        fr[32 + r] = __builtin_bit_cast(uint4, hi);
                    } else {
                        __bf16 z1, z2, z3;
                        split3(zs[r], z1, z2, z3);
                        const __bf16 zero = (__bf16)0.0f;
                        const nn_bf16x8 hi = {y1, y3, y2, y1, z1, z2, z1, z3};
                        const nn_bf16x8 lo1 = {z2, z1, n1, n2, n3, zero, zero, zero};
                        const nn_bf16x8 hi1 = {zero, zero, zero, zero, zero, zero, zero, zero};
                        fr[32 + r] = __builtin_bit_cast(uint4, hi);
                        uint4 *fr1 = &frag[KS - 1][ch][p4];
                        fr1[r] = __builtin_bit_cast(uint4, lo1);
                        fr1[32 + r] = __builtin_bit_cast(uint4, hi1);
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int g = 0; g < NNM_GROUPS; ++g) w[g] = 0u;
            // (tried, no gain: a software pipeline one chunk deep -- the MFMAs of chunk c + 1 issued between the reductions of
            // chunk c, pinned with sched_group_barrier: 173-199 VGPRs, two waves per SIMD instead of three, 20 % slower)
            // t = min(thr, chunk minimum) by a tree of v_min3 that starts from thr (a canonical fp32 value, so that no input of the
            // tree needs quieting); the chunk is flagged when t < thr -- the sign bit of t - thr, shifted into the flag word by one
            // v_alignbit (a compare + select through a lane mask costs 3 ns per MFMA more: scripts/ubench/mfma_valu.hip) -- and
            // min(brun, t) is the new bound either way.  The threshold follows the bound every OTHER chunk: a stale threshold is
            // a larger one (thr is monotone in the bound), which flags a superset, and the fma is one vector instruction less
            // per MFMA on a loop the vector pipe binds (the matrix pipe does NOT hide it: 17.7 ns per MFMA and SIMD alone,
            // 28.8 with the eight v_min3, 36.4 / 30.9 with the bookkeeping before / after this change).
            auto reduce = [&](const nn_f32x16 &acc, int g, bool refresh) {
                auto m3 = [](float a, float b, float c) { return __builtin_fminf(__builtin_fminf(a, b), c); };
                const float m0 = m3(thr[g], acc[0], acc[1]), m1 = m3(acc[2], acc[3], acc[4]), m2 = m3(acc[5], acc[6], acc[7]);
                const float m4 = m3(acc[8], acc[9], acc[10]), m5 = m3(acc[11], acc[12], acc[13]);
                const float n0 = m3(m0, m1, m2), n1 = m3(m4, m5, acc[14]);
                const float t = m3(n0, n1, acc[15]);
                w[g] = __builtin_amdgcn_alignbit(w[g], __float_as_uint(t - thr[g]), 31);      // chunk c ends up in bit 31 - c
                brun[g] = __builtin_fminf(brun[g], t);
                if (refresh) thr[g] = __builtin_fmaf(brun[g], kp1, c2[g]);
            };
            uint4 af_next[KS];
#pragma unroll
            for (int k = 0; k < KS; ++k) af_next[k] = frag[k][0][lane];
#pragma unroll 2
            for (int c = 0; c < NCH; ++c) {
                nn_bf16x8 af[KS];
#pragma unroll
                for (int k = 0; k < KS; ++k) {
                    af[k] = __builtin_bit_cast(nn_bf16x8, af_next[k]);
                    af_next[k] = frag[k][(c + 1) & (NCH - 1)][lane];            // next chunk's fragment in flight behind this chunk's MFMAs
                }
                const bool refresh = (c & 1) != 0;
                // two (chains of) MFMAs in flight per wave (32 accumulator registers)
#pragma unroll
                for (int h2 = 0; h2 < NNM_GROUPS; h2 += 2) {
                    nn_f32x16 acc0 = mfma_32x32x16_bf16_c0(af[0], bfr[0][h2]);
                    nn_f32x16 acc1 = mfma_32x32x16_bf16_c0(af[0], bfr[0][h2 + 1]);
                    if constexpr (KS == 2) {
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[KS - 1], bfr[KS - 1][h2], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[KS - 1], bfr[KS - 1][h2 + 1], acc1, 0, 0, 0);
                    }
                    reduce(acc0, h2, refresh);
                    reduce(acc1, h2 + 1, refresh);
                }
            }
            // ---- flags of the two lanes that share a point, then the exact re-scan of this sub-tile's flagged chunks while
            // it is in LDS (chunks ascending, tiles ascending, strict '<': the lowest index among equal distances)
            unsigned wo[2];
            {
                unsigned wf[NNM_GROUPS];
#pragma unroll
                for (int g = 0; g < NNM_GROUPS; ++g) {
                    // (NCH < 32: the flags sit in the top NCH bits, in chunk order from bit 31 down, once the word has been shifted NCH times)
                    const unsigned wg = NCH == 32 ? w[g] : (w[g] << (32 - NCH));
                    wf[g] = wg | (unsigned)__shfl_xor((int)wg, 32, 64);
                }
                wo[0] = half ? wf[2] : wf[0];
                wo[1] = half ? wf[3] : wf[1];
            }
            // (one loop over the flags of both points a lane owns: the wave leaves it after max over lanes of (flags of point 0 +
            // flags of point 1) rounds instead of the sum of the two maxima)
            while (__any((wo[0] | wo[1]) != 0u)) {
                if ((wo[0] | wo[1]) != 0u) {
                    const bool second = wo[0] == 0u;
                    const unsigned ww = second ? wo[1] : wo[0];
                    const int c = __clz((int)ww);
                    const unsigned rest = ww & ~(0x80000000u >> c);
                    wo[0] = second ? wo[0] : rest;
                    wo[1] = second ? rest : wo[1];
                    float pq[DIM];
                    pq[0] = second ? pox[1] : pox[0];
                    pq[1] = second ? poy[1] : poy[0];
                    if constexpr (DIM == 3) pq[DIM - 1] = second ? poz[1] : poz[0];
                    const int o0 = c * 32;
                    float best = INFINITY;
                    int bj = 0;
#pragma unroll
                    for (int h = 0; h < 8; ++h) {
                        const float4 vx = *reinterpret_cast<const float4 *>(&lt[0][o0 + h * 4]);
                        const float4 vy = *reinterpret_cast<const float4 *>(&lt[1][o0 + h * 4]);
                        float4 vz = make_float4(0.f, 0.f, 0.f, 0.f);
                        if constexpr (DIM == 3) vz = *reinterpret_cast<const float4 *>(&lt[DIM - 1][o0 + h * 4]);
                        const float d0 = nn_dist<DIM>(vx.x, vy.x, vz.x, pq), d1 = nn_dist<DIM>(vx.y, vy.y, vz.y, pq);
                        const float d2 = nn_dist<DIM>(vx.z, vy.z, vz.z, pq), d3 = nn_dist<DIM>(vx.w, vy.w, vz.w, pq);
                        if (d0 < best) { best = d0; bj = h * 4 + 0; }
                        if (d1 < best) { best = d1; bj = h * 4 + 1; }
                        if (d2 < best) { best = d2; bj = h * 4 + 2; }
                        if (d3 < best) { best = d3; bj = h * 4 + 3; }
                    }
                    const int jn = t * TT + o0 + bj;
                    if (!second && best < cur[0]) { cur[0] = best; jj[0] = jn; }
                    if (second && best < cur[1]) { cur[1] = best; jj[1] = jn; }
                }
            }
        }

#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int i = pidx[q];
            if (i >= N) continue;
            if (!(cur[q] < INFINITY) && tu != 0) continue;
            // A seeded point's answer is never farther than its seed target, whose own unit finds and writes it: a unit that
            // holds neither the seed target nor anything as close has nothing to add to the atomic minimum ('<=': an equally
            // distant target with a lower index must still get its say).  13.7 -> 1.5 MB of 8-byte atomics per launch.
            const bool holds_seed = jso[q] >= t0 * NN_TILE && jso[q] < t1 * NN_TILE;
            if (jso[q] >= 0 && !holds_seed && !(cur[q] <= dso[q])) continue;
            if (holds_seed && !(cur[q] <= dso[q])) {       // (cannot happen while the filter holds; keeps the key armed whatever happens)
                cur[q] = dso[q];
                jj[q] = jso[q];
            }
            const unsigned long long key =
                ((unsigned long long)__float_as_uint(cur[q]) << 32) | (unsigned long long)(unsigned)jj[q];
            atomicMin(&packed[(size_t)b * N + i], key);
        }
    }
}

// The first ICP iteration has no previous correspondent to start the filter's bound from, and a bound that starts at infinity
// flags a "record" sequence of chunks in every unit (189 us per launch against 130 for a seeded one).  This pass gives it a
// seed: the nearest of every 64th target.  A seed only bounds the search -- the correspondences stay the exhaustive scan's --
// so its own arithmetic is free: packed fp32 (two samples per instruction), and the sample's number in the low 10 bits of
// the distance so that one unsigned minimum tracks value and index (distances are >= 0: their bit patterns order like the
// values).  Source blocks the scan skips (all-zero rows behind the first zero row) are skipped here too.  Measured (B = 32,
// survey density): 18 us for the pass, the first launch's scan 189 -> ~150 us behind it: 189 -> 180 us in all (every 32nd target
// with exact nn_dist: 35 us for the pass, no gain; 64-thread blocks: 21 us).
constexpr int NN_COARSE_STRIDE = 64, NN_COARSE_TILE = 1024, NN_COARSE_THREADS = 256;
typedef __attribute__((ext_vector_type(2))) float nn_f32x2;
template <int DIM>
__global__ __launch_bounds__(NN_COARSE_THREADS) void nn_coarse_seed_kernel(const float *__restrict__ src, const float *__restrict__ tgtp,
                                                             const float *__restrict__ Tk, const int32_t *__restrict__ active,
                                                             const int32_t *__restrict__ allzero, const int32_t *__restrict__ zrep,
                                                             int nn_pts, int nsb, int N, int Mpad, const float *__restrict__ dec,
                                                             int32_t *__restrict__ seed)
{
    __shared__ __attribute__((aligned(16))) float st[DIM][NN_COARSE_TILE];
    const int b = blockIdx.y;
    if (active != nullptr && active[b] == 0) return;
    if (allzero != nullptr) {
        const int sb = (blockIdx.x * NN_COARSE_THREADS) / nn_pts;
        if (sb < nsb && allzero[(size_t)b * nsb + sb] != 0 && zrep[b] < sb * nn_pts) return;
    }
    const int i = blockIdx.x * NN_COARSE_THREADS + threadIdx.x;
    float T[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) T[q] = Tk[(size_t)b * 16 + q];
    float p[DIM] = {};
    if (i < N) {
        const float *sp = src + ((size_t)b * N + i) * 3;
        const float s[3] = {sp[0], sp[1], sp[2]};
        transform_point<DIM>(T, s, p);
    }
    const float *tb = tgtp + (size_t)b * DIM * Mpad;
    const int ns = Mpad / NN_COARSE_STRIDE;
    unsigned best = 0x7f800000u;          // (+inf: nothing found)
    int best_tile = 0;
    const nn_f32x2 npx = {-p[0], -p[0]}, npy = {-p[1], -p[1]}, npz = {-p[DIM - 1], -p[DIM - 1]};
    for (int s0 = 0; s0 < ns; s0 += NN_COARSE_TILE) {
        __syncthreads();
        for (int q = threadIdx.x; q < NN_COARSE_TILE; q += NN_COARSE_THREADS) {
            const int sidx = s0 + q;
#pragma unroll
            for (int c = 0; c < DIM; ++c)
                st[c][q] = sidx >= ns ? 3e18f
                                      : (dec != nullptr ? dec[((size_t)b * DIM + c) * ns + sidx] : tb[(size_t)c * Mpad + (size_t)sidx * NN_COARSE_STRIDE]);
        }
        __syncthreads();
        const int cnt = min(NN_COARSE_TILE, ns - s0);
        unsigned tb_best = 0x7f800000u;
        for (int q = 0; q < cnt; q += 4) {
            const float4 vx = *reinterpret_cast<const float4 *>(&st[0][q]);
            const float4 vy = *reinterpret_cast<const float4 *>(&st[1][q]);
            const nn_f32x2 dx0 = nn_f32x2{vx.x, vx.y} + npx, dx1 = nn_f32x2{vx.z, vx.w} + npx;
            const nn_f32x2 dy0 = nn_f32x2{vy.x, vy.y} + npy, dy1 = nn_f32x2{vy.z, vy.w} + npy;
            nn_f32x2 d0 = dx0 * dx0, d1 = dx1 * dx1;
            d0 = __builtin_elementwise_fma(dy0, dy0, d0);
            d1 = __builtin_elementwise_fma(dy1, dy1, d1);
            if (DIM == 3) {
                const float4 vz = *reinterpret_cast<const float4 *>(&st[DIM - 1][q]);
                const nn_f32x2 dz0 = nn_f32x2{vz.x, vz.y} + npz, dz1 = nn_f32x2{vz.z, vz.w} + npz;
                d0 = __builtin_elementwise_fma(dz0, dz0, d0);
                d1 = __builtin_elementwise_fma(dz1, dz1, d1);
            }
            const unsigned k0 = (__float_as_uint(d0[0]) & 0xfffffc00u) | (unsigned)q;
            const unsigned k1 = (__float_as_uint(d0[1]) & 0xfffffc00u) | (unsigned)(q + 1);
            const unsigned k2 = (__float_as_uint(d1[0]) & 0xfffffc00u) | (unsigned)(q + 2);
            const unsigned k3 = (__float_as_uint(d1[1]) & 0xfffffc00u) | (unsigned)(q + 3);
            tb_best = min(min(tb_best, min(k0, k1)), min(k2, k3));       // (a NaN's pattern is above +inf: never the minimum)
        }
        if (tb_best < (best & 0xfffffc00u)) {
            best = tb_best;
            best_tile = s0;
        }
    }
    if (i < N) seed[(size_t)b * N + i] = best >= 0x7f800000u ? -1 : (best_tile + (int)(best & 0x3ffu)) * NN_COARSE_STRIDE;
}

constexpr unsigned long long NN_KEY_INIT = ~0ull;

__global__ void nn_unpack_kernel(const unsigned long long *__restrict__ packed, int n, int32_t *__restrict__ idx,
                                 float *__restrict__ d2)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = packed[i];
    idx[i] = (int32_t)(unsigned)(key & 0xffffffffull);
    d2[i] = __uint_as_float((unsigned)(key >> 32));
}


// ------------------------------------------------------------------------------------------
// I2, accelerated form: EXACT nearest neighbour through a uniform 2-D grid
// over the target's x,y.  It returns bit for bit what the brute-force scan returns — the same
// nn_dist() arithmetic on the same coordinates, ties to the lowest original index — but only
// visits the cells that can hold the answer: rings of cells around the query are scanned until
// the best distance is provably smaller than anything an unvisited ring can offer (a point in a
// cell at Chebyshev ring r+1 is at least r cells away; targets/queries outside the grid are
// clamped to the border cells, which only makes them farther than the bound).  A query that is
// still unresolved after GRID_RMAX rings scans every target.  The grid is built once per icp()
// call (the target does not move between iterations).
constexpr int GRID_N = 128;
constexpr int GRID_NC = GRID_N * GRID_N;
constexpr float GRID_CELL = 2.0f;
constexpr float GRID_ORG = -128.0f;
constexpr int GRID_RMAX = 24;

__device__ __forceinline__ int grid_coord(float v)
{
    const float f = floorf((v - GRID_ORG) / GRID_CELL);
    return (int)fminf(fmaxf(f, 0.f), (float)(GRID_N - 1));
}

__global__ void grid_count_kernel(const float *__restrict__ tgt, int M, int cols, int32_t *__restrict__ counts)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (j >= M) return;
    const float *t = tgt + ((size_t)b * M + j) * cols;
    const int cell = grid_coord(t[1]) * GRID_N + grid_coord(t[0]);
    atomicAdd(&counts[(size_t)b * GRID_NC + cell], 1);
}

__global__ __launch_bounds__(256) void grid_scan_kernel(const int32_t *__restrict__ counts, int32_t *__restrict__ starts)
{
    __shared__ int sm[4];
    const int b = blockIdx.x;
    constexpr int L = GRID_NC / 256;
    const int32_t *c = counts + (size_t)b * GRID_NC + threadIdx.x * L;
    int s = 0;
    for (int i = 0; i < L; ++i) s += c[i];
    // block exclusive scan of 256 partial sums
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = s;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    if (lane == 63) sm[wv] = inc;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wv; ++w) base += sm[w];
    int run = base + inc - s;
    int32_t *o = starts + (size_t)b * (GRID_NC + 1) + threadIdx.x * L;
    for (int i = 0; i < L; ++i) {
        o[i] = run;
        run += c[i];
    }
    if (threadIdx.x == 255) starts[(size_t)b * (GRID_NC + 1) + GRID_NC] = run;
}

__global__ void grid_fill_kernel(const float *__restrict__ tgt, int M, int cols, int dim, const int32_t *__restrict__ starts,
                                 int32_t *__restrict__ cursor, float4 *__restrict__ sorted)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (j >= M) return;
    const float *t = tgt + ((size_t)b * M + j) * cols;
    const int cell = grid_coord(t[1]) * GRID_N + grid_coord(t[0]);
    const int pos = starts[(size_t)b * (GRID_NC + 1) + cell] + atomicAdd(&cursor[(size_t)b * GRID_NC + cell], 1);
    sorted[(size_t)b * M + pos] = make_float4(t[0], t[1], dim == 3 ? t[2] : 0.f, __int_as_float(j));
}

template <int DIM>
__global__ __launch_bounds__(256) void grid_nn_kernel(const float *__restrict__ src, const float *__restrict__ Tk,
                                                      const int32_t *__restrict__ active,
                                                      const int32_t *__restrict__ starts,
                                                      const float4 *__restrict__ sorted, int N, int M,
                                                      const float *__restrict__ tgt, int cols,
                                                      const int32_t *__restrict__ prev_idx,
                                                      unsigned long long *__restrict__ packed)
{
    const int b = blockIdx.y;
    if (active != nullptr && active[b] == 0) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float T[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) T[q] = Tk[(size_t)b * 16 + q];
    const float *sp = src + ((size_t)b * N + i) * 3;
    const float s[3] = {sp[0], sp[1], sp[2]};
    float p[DIM];
    transform_point<DIM>(T, s, p);
    const int cx = grid_coord(p[0]), cy = grid_coord(p[1]);
    const int32_t *st = starts + (size_t)b * (GRID_NC + 1);
    const float4 *pts = sorted + (size_t)b * M;
    float best = INFINITY;
    int bi = 0x7fffffff;

    // candidates are fetched eight at a time (independent 16-byte loads) before they are compared:
    // the search is latency-bound, not ALU-bound
    auto scan = [&](int k0, int k1) {
        for (int k = k0; k < k1; k += 8) {
            float4 t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = pts[min(k + u, k1 - 1)];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float d = nn_dist<DIM>(t[u].x, t[u].y, t[u].z, p);
                const int j = __float_as_int(t[u].w);
                if (d < best || (d == best && j < bi)) {
                    best = d;
                    bi = j;
                }
            }
        }
    };

    auto scan_square = [&](int r) {
        const int y0 = max(cy - r, 0), y1 = min(cy + r, GRID_N - 1);
        const int x0 = max(cx - r, 0), x1 = min(cx + r, GRID_N - 1);
        int k0 = st[y0 * GRID_N + x0], k1 = st[y0 * GRID_N + x1 + 1];
        for (int y = y0; y <= y1; ++y) {
            const int yn = min(y + 1, y1);
            const int n0 = st[yn * GRID_N + x0], n1 = st[yn * GRID_N + x1 + 1];   // next row's range in flight
            scan(k0, k1);
            k0 = n0;
            k1 = n1;
        }
    };

    bool done = false;
    if (prev_idx != nullptr) {
        // the previous iteration's correspondent bounds the search: every target at most that far
        // away (the answer and all its ties) lies within r cells of the query's cell
        const float *tp = tgt + ((size_t)b * M + prev_idx[(size_t)b * N + i]) * cols;
        const float u = nn_dist<DIM>(tp[0], tp[1], DIM == 3 ? tp[2] : 0.f, p);
        const int r = (int)floorf((sqrtf(u) + 1e-3f) / GRID_CELL) + 1;
        if (r <= GRID_RMAX) {
            scan_square(r);
            done = true;
        }
    }
    // growing squares of cells around the query (inner cells are simply seen again: harmless);
    // after the square of radius r everything unvisited is at least r cells away
    const int radii[8] = {1, 2, 3, 5, 8, 12, 17, GRID_RMAX};
    for (int ri = 0; ri < 8 && !done; ++ri) {
        const int r = radii[ri];
        scan_square(r);
        const float lim = (float)r * GRID_CELL - 1e-3f;   // 1 mm of slack for the float cell assignment
        done = best < lim * lim;
    }
    if (!done) {   // far from every target: exhaustive scan (still exact)
        best = INFINITY;
        bi = 0x7fffffff;
        scan(0, M);
    }
    packed[(size_t)b * N + i] = ((unsigned long long)__float_as_uint(best) << 32) | (unsigned long long)(unsigned)bi;
}

// ------------------------------------------------------------------------------------------
// Target normals (DESIGN.md §3 "N1"): the k nearest valid rows of a cloud to each of its own rows, EXACT, through the
// same grid, then the smallest eigenpair of their covariance.  Serves the normals columns of the reference's map tensor
// (mm_masking/icp_weight_dataset.py:395-398), which upstream come out of vtr3 and nothing here could produce.
//
// One point per thread, taken in the grid's cell order (neighbouring lanes walk the same cells; results go to the row's
// own index, so the order is invisible).  The top-k is an array of packed keys (bits(d2) << 32 | index: integer order =
// nearer first, ties to the lowest index) held in registers in DESCENDING order, so that the worst kept key is the static
// slot 0: a candidate below it replaces it and sinks through k - 1 unrolled compare-exchanges.  Every index into the
// array is a compile-time constant; slots >= k are switched off by predicates on that constant (a run-time index would
// put the array into scratch memory).
//
// Unlike grid_nn_kernel's minimum, a top-k must not see a candidate twice, so each radius scans only the annulus that
// the previous square left out (full rows above and below it, two side segments beside it).  The stopping rule is that
// kernel's: after the square of radius r every unvisited row is at least r cells away in x or in y -- rows and queries
// outside the +-128 m grid are clamped into the border cells, which only puts them farther away than the bound, so a
// cloud far from the origin costs time, never exactness -- and the search ends when the k-th distance is below that
// bound (1 mm of slack for the float cell assignment) or the bound has passed max_radius.  A query that GRID_RMAX rings
// do not settle starts over and scans every row.
constexpr int KNN_THREADS = 256;
constexpr int KNN_JACOBI_SWEEPS = 8;
constexpr unsigned long long KNN_EMPTY = ~0ull;

template <int DIM>
__device__ __forceinline__ bool knn_is_pad(float x, float y, float z, float pad_val)
{
    bool pad = fabsf(x) >= pad_val || fabsf(y) >= pad_val;
    if constexpr (DIM == 3) pad = pad || fabsf(z) >= pad_val;
    return pad_val > 0.f && pad;
}

// One Jacobi rotation of a symmetric 3x3 in the (p,q) plane; r is the third index.  (Golub & Van Loan, Alg. 8.4.1.)
__device__ __forceinline__ void jacobi_rot(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p,
                                           double &v0q, double &v1p, double &v1q, double &v2p, double &v2q)
{
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app -= t * apq;
    aqq += t * apq;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp;
    arq = rq;
    const double a0 = c * v0p - s * v0q, b0 = s * v0p + c * v0q;
    const double a1 = c * v1p - s * v1q, b1 = s * v1p + c * v1q;
    const double a2 = c * v2p - s * v2q, b2 = s * v2p + c * v2q;
    v0p = a0, v0q = b0, v1p = a1, v1q = b1, v2p = a2, v2q = b2;
}

template <int DIM, int KC>
__global__ __launch_bounds__(KNN_THREADS) void knn_normals_kernel(
    const float *__restrict__ pts_in, int M, int cols, int k, float max_radius, float pad_val,
    const float *__restrict__ viewpoint, const int32_t *__restrict__ starts, const float4 *__restrict__ sorted,
    float *__restrict__ normals, float *__restrict__ curvature, int32_t *__restrict__ count_out, int32_t *__restrict__ nbr_idx)
{
    const int b = blockIdx.y;
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= M) return;
    const float4 *pts = sorted + (size_t)b * M;
    const float4 q = pts[s];
    const int row = __float_as_int(q.w);
    const size_t orow = (size_t)b * M + row;
    if (knn_is_pad<DIM>(q.x, q.y, q.z, pad_val)) {
        normals[orow * 3 + 0] = 0.f;
        normals[orow * 3 + 1] = 0.f;
        normals[orow * 3 + 2] = 0.f;
        if (curvature != nullptr) curvature[orow] = 0.f;
        if (count_out != nullptr) count_out[orow] = 0;
        if (nbr_idx != nullptr)
            for (int j = 0; j < k; ++j) nbr_idx[orow * k + j] = -1;
        return;
    }
    float p[DIM];
    p[0] = q.x;
    p[1] = q.y;
    if constexpr (DIM == 3) p[2] = q.z;
    const int cx = grid_coord(p[0]), cy = grid_coord(p[1]);
    const int32_t *st = starts + (size_t)b * (GRID_NC + 1);
    const bool use_r = max_radius > 0.f;
    const float r2 = max_radius * max_radius;

    unsigned long long a[KC];   // descending: a[0] is the worst kept key, KNN_EMPTY while fewer than k are kept
#pragma unroll
    for (int j = 0; j < KC; ++j) a[j] = KNN_EMPTY;

    // ONE scan site (the unrolled top-k update is long, and a second copy of it would double the kernel): step 0..7 scan the
    // annulus of radii[step], step 8 is the exhaustive scan, written as a single "row" that spans every sorted row.
    // Candidates are fetched eight at a time (independent 16-byte loads), as in grid_nn_kernel; the tail's repeats of the
    // last row are switched off, not offered twice.
    bool done = false;
    int rp = -1;   // the square of radius rp has been scanned
    for (int step = 0; step <= 8 && !done; ++step) {
        const bool all = step == 8;   // fewer than k rows within GRID_RMAX rings: start over, scan every row (still exact)
        const int r = step == 0 ? 1 : step == 1 ? 2 : step == 2 ? 3 : step == 3 ? 5 : step == 4 ? 8 : step == 5 ? 12 : step == 6 ? 17 : GRID_RMAX;
        if (all) {
#pragma unroll
            for (int j = 0; j < KC; ++j) a[j] = KNN_EMPTY;
        }
        for (int rc = 0; rc < (all ? 1 : 4); ++rc) {
            // rows above the old square (at first, rp = -1: down to the query's own row), rows below it, the two segments
            // beside it; clipped to the grid
            int x0 = rc == 3 ? cx + rp + 1 : cx - r, x1 = rc == 2 ? cx - rp - 1 : cx + r;
            int y0 = rc == 0 ? cy - r : rc == 1 ? cy + max(rp, 0) + 1 : cy - rp, y1 = rc == 0 ? cy - rp - 1 : rc == 1 ? cy + r : cy + rp;
            x0 = max(x0, 0), y0 = max(y0, 0), x1 = min(x1, GRID_N - 1), y1 = min(y1, GRID_N - 1);
            if (all) x0 = x1 = y0 = y1 = 0;
            if (x0 > x1) continue;
            for (int y = y0; y <= y1; ++y) {
                const int k0 = all ? 0 : st[y * GRID_N + x0], k1 = all ? M : st[y * GRID_N + x1 + 1];
                for (int kk = k0; kk < k1; kk += 8) {
                    float4 t[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) t[u] = pts[min(kk + u, k1 - 1)];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const float d = nn_dist<DIM>(t[u].x, t[u].y, t[u].z, p);
                        const unsigned long long key =
                            ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)__float_as_uint(t[u].w);
                        if (kk + u < k1 && !knn_is_pad<DIM>(t[u].x, t[u].y, t[u].z, pad_val) && !(use_r && d > r2) && key < a[0]) {
                            a[0] = key;
#pragma unroll
                            for (int j = 0; j + 1 < KC; ++j) {
                                const bool sw = (j + 1 < k) && a[j] < a[j + 1];
                                const unsigned long long hi = sw ? a[j + 1] : a[j], lo = sw ? a[j] : a[j + 1];
                                a[j] = hi;
                                a[j + 1] = lo;
                            }
                        }
                    }
                }
            }
        }
        rp = r;
        const float lim = (float)r * GRID_CELL - 1e-3f;   // 1 mm of slack for the float cell assignment
        done = all || (a[0] != KNN_EMPTY && __uint_as_float((unsigned)(a[0] >> 32)) < lim * lim) || (use_r && lim > max_radius);
    }

    // ---- neighbours in key order = slots k-1 .. 0; the empty slots are the leading ones
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < KC; ++j) cnt += (j < k && a[j] != KNN_EMPTY) ? 1 : 0;
    if (count_out != nullptr) count_out[orow] = cnt;
    if (nbr_idx != nullptr) {
#pragma unroll
        for (int j = 0; j < KC; ++j)
            if (j < k) nbr_idx[orow * k + (k - 1 - j)] = a[j] != KNN_EMPTY ? (int32_t)(unsigned)a[j] : -1;
    }
    float n0 = 0.f, n1 = 0.f, n2 = 0.f, curv = 0.f;
    if (cnt >= 3) {
        const float *base = pts_in + (size_t)b * M * cols;
        // two passes in fp64 over the fp32 coordinates, in key order
        double mx = 0.0, my = 0.0, mz = 0.0;
#pragma unroll
        for (int j = KC - 1; j >= 0; --j) {
            if (j < k && a[j] != KNN_EMPTY) {
                const float *t = base + (size_t)(unsigned)a[j] * cols;
                mx += (double)t[0];
                my += (double)t[1];
                if constexpr (DIM == 3) mz += (double)t[2];
            }
        }
        // divided, not scaled by 1 / cnt: the centroid of rows that share a coordinate is then that coordinate exactly
        const double inv = 1.0 / (double)cnt;
        mx /= (double)cnt, my /= (double)cnt, mz /= (double)cnt;
        double cxx = 0.0, cxy = 0.0, cxz = 0.0, cyy = 0.0, cyz = 0.0, czz = 0.0;
#pragma unroll
        for (int j = KC - 1; j >= 0; --j) {
            if (j < k && a[j] != KNN_EMPTY) {
                const float *t = base + (size_t)(unsigned)a[j] * cols;
                const double dx = (double)t[0] - mx, dy = (double)t[1] - my;
                cxx += dx * dx;
                cxy += dx * dy;
                cyy += dy * dy;
                if constexpr (DIM == 3) {
                    const double dz = (double)t[2] - mz;
                    cxz += dx * dz;
                    cyz += dy * dz;
                    czz += dz * dz;
                }
            }
        }
        cxx *= inv, cxy *= inv, cyy *= inv, cxz *= inv, cyz *= inv, czz *= inv;
        double ex, ey, ez = 0.0, lmin, lsum;
        if constexpr (DIM == 2) {
            // closed form: lambda_min = (a + c) / 2 - sqrt(((a - c) / 2)^2 + b^2); its eigenvector is (b, l - a) and also
            // (l - c, b) -- the longer of the two is the well-conditioned one
            const double h = 0.5 * (cxx - cyy), root = cxy == 0.0 ? fabs(h) : sqrt(h * h + cxy * cxy);
            lmin = 0.5 * (cxx + cyy) - root;
            lsum = cxx + cyy;
            const double u0 = cxy, u1 = lmin - cxx, w0 = lmin - cyy, w1 = cxy;
            const bool first = u0 * u0 + u1 * u1 >= w0 * w0 + w1 * w1;
            ex = first ? u0 : w0;
            ey = first ? u1 : w1;
            if (ex == 0.0 && ey == 0.0) ex = 1.0;   // isotropic: every direction is an eigenvector
        } else {
            // cyclic Jacobi, KNN_JACOBI_SWEEPS sweeps of the rotations (0,1), (0,2), (1,2): convergence is quadratic once the
            // off-diagonal norm is small against the gaps, which a 3x3 reaches within three or four sweeps (off/||A|| goes
            // ~1e-1, 1e-2, 1e-4, 1e-8, < 1e-16), so 8 leaves several sweeps that rotate by nothing
            double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
            for (int sweep = 0; sweep < KNN_JACOBI_SWEEPS; ++sweep) {
                jacobi_rot(cxx, cyy, cxy, cxz, cyz, v00, v01, v10, v11, v20, v21);
                jacobi_rot(cxx, czz, cxz, cxy, cyz, v00, v02, v10, v12, v20, v22);
                jacobi_rot(cyy, czz, cyz, cxy, cxz, v01, v02, v11, v12, v21, v22);
            }
            lsum = cxx + cyy + czz;
            // the smallest eigenvalue's column (ties to the lower index), by selects: an indexed pick would go through scratch
            const bool s1 = cyy < cxx;
            const double l01 = s1 ? cyy : cxx;
            const bool s2 = czz < l01;
            lmin = s2 ? czz : l01;
            ex = s2 ? v02 : (s1 ? v01 : v00);
            ey = s2 ? v12 : (s1 ? v11 : v10);
            ez = s2 ? v22 : (s1 ? v21 : v20);
        }
        const double nrm = sqrt(ex * ex + ey * ey + ez * ez);
        ex /= nrm, ey /= nrm, ez /= nrm;
        double vx = 0.0, vy = 0.0, vz = 0.0;
        if (viewpoint != nullptr) vx = (double)viewpoint[b * 3 + 0], vy = (double)viewpoint[b * 3 + 1], vz = (double)viewpoint[b * 3 + 2];
        double dot = ex * (vx - (double)p[0]) + ey * (vy - (double)p[1]);
        if constexpr (DIM == 3) dot += ez * (vz - (double)p[2]);
        if (dot < 0.0) ex = -ex, ey = -ey, ez = -ez;
        n0 = (float)ex, n1 = (float)ey, n2 = (float)ez;
        lmin = fmax(lmin, 0.0);
        curv = lsum > 0.0 ? (float)(lmin / lsum) : 0.f;
    }
    normals[orow * 3 + 0] = n0;
    normals[orow * 3 + 1] = n1;
    normals[orow * 3 + 2] = n2;
    if (curvature != nullptr) curvature[orow] = curv;
}

// ------------------------------------------------------------------------------------------
// I2' (DESIGN.md §3): the k (2..8) nearest target rows of every transformed source point, EXACT, for the soft
// correspondences.  grid_nn_kernel's query (one transformed source point per thread, the pair's pose, the active flag) with
// knn_normals_kernel's search: the top-8 packed keys in registers in descending order, every index a compile-time constant,
// slots >= k switched off by predicates, each radius scanning only the annulus the previous square left out, the search over
// once the k-th distance is below the ring bound, the exhaustive scan after GRID_RMAX.  No row is special: target_pad_val
// rows are simply far away.  keys (B,N,k) in key order -- ascending d, ties to the lowest index -- so slot 0 is the
// correspondent the hard searches return.  M >= k (the entries check it), so the exhaustive scan fills every slot.
constexpr int SOFT_KMAX = 8;

template <int DIM>
__global__ __launch_bounds__(KNN_THREADS) void grid_knn_kernel(const float *__restrict__ src, const float *__restrict__ Tk,
                                                               const int32_t *__restrict__ active,
                                                               const int32_t *__restrict__ starts,
                                                               const float4 *__restrict__ sorted, int N, int M, int k,
                                                               unsigned long long *__restrict__ keys)
{
    constexpr int KC = SOFT_KMAX;
    const int b = blockIdx.y;
    if (active != nullptr && active[b] == 0) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float T[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) T[q] = Tk[(size_t)b * 16 + q];
    const float *sp = src + ((size_t)b * N + i) * 3;
    const float s[3] = {sp[0], sp[1], sp[2]};
    float p[DIM];
    transform_point<DIM>(T, s, p);
    const int cx = grid_coord(p[0]), cy = grid_coord(p[1]);
    const int32_t *st = starts + (size_t)b * (GRID_NC + 1);
    const float4 *pts = sorted + (size_t)b * M;

    unsigned long long a[KC];   // descending: a[0] is the worst kept key, KNN_EMPTY while fewer than k are kept
#pragma unroll
    for (int j = 0; j < KC; ++j) a[j] = KNN_EMPTY;

    // one scan site, as in knn_normals_kernel: steps 0..7 scan the annulus of their radius, step 8 every row
    bool done = false;
    int rp = -1;   // the square of radius rp has been scanned
    for (int step = 0; step <= 8 && !done; ++step) {
        const bool all = step == 8;
        const int r = step == 0 ? 1 : step == 1 ? 2 : step == 2 ? 3 : step == 3 ? 5 : step == 4 ? 8 : step == 5 ? 12 : step == 6 ? 17 : GRID_RMAX;
        if (all) {
#pragma unroll
            for (int j = 0; j < KC; ++j) a[j] = KNN_EMPTY;
        }
        for (int rc = 0; rc < (all ? 1 : 4); ++rc) {
            int x0 = rc == 3 ? cx + rp + 1 : cx - r, x1 = rc == 2 ? cx - rp - 1 : cx + r;
            int y0 = rc == 0 ? cy - r : rc == 1 ? cy + max(rp, 0) + 1 : cy - rp, y1 = rc == 0 ? cy - rp - 1 : rc == 1 ? cy + r : cy + rp;
            x0 = max(x0, 0), y0 = max(y0, 0), x1 = min(x1, GRID_N - 1), y1 = min(y1, GRID_N - 1);
            if (all) x0 = x1 = y0 = y1 = 0;
            if (x0 > x1) continue;
            for (int y = y0; y <= y1; ++y) {
                const int k0 = all ? 0 : st[y * GRID_N + x0], k1 = all ? M : st[y * GRID_N + x1 + 1];
                for (int kk = k0; kk < k1; kk += 8) {
                    float4 t[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) t[u] = pts[min(kk + u, k1 - 1)];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const float d = nn_dist<DIM>(t[u].x, t[u].y, t[u].z, p);
                        const unsigned long long key =
                            ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)__float_as_uint(t[u].w);
                        if (kk + u < k1 && key < a[0]) {
                            a[0] = key;
#pragma unroll
                            for (int j = 0; j + 1 < KC; ++j) {
                                const bool sw = (j + 1 < k) && a[j] < a[j + 1];
                                const unsigned long long hi = sw ? a[j + 1] : a[j], lo = sw ? a[j] : a[j + 1];
                                a[j] = hi;
                                a[j + 1] = lo;
                            }
                        }
                    }
                }
            }
        }
        rp = r;
        const float lim = (float)r * GRID_CELL - 1e-3f;   // 1 mm of slack for the float cell assignment
        done = all || (a[0] != KNN_EMPTY && __uint_as_float((unsigned)(a[0] >> 32)) < lim * lim);
    }
    // key order = slots k-1 .. 0
    unsigned long long *out = keys + ((size_t)b * N + i) * k;
#pragma unroll
    for (int j = 0; j < KC; ++j)
        if (j < k) out[k - 1 - j] = a[j];
}

// ------------------------------------------------------------------------------------------
// I3 + I4 per-point terms (oracle: per_point_terms).
template <int DIM, int TYPE>
struct PointTerms {
    static constexpr int P = (DIM == 2) ? 3 : 6;
    static constexpr int NR = (TYPE == MMK_ICP_PT2PT) ? DIM : 1;
    float s[3];
    float p[DIM];
    float ev[DIM];
    float n[DIM];
    float J[NR][P];
    float er[NR];
    float d2, r2, keep, rho, w, omega;
    float d, th;        // soft gate only (I3'): distance and tanh of the gate's argument, for the backward
};

// The trim gate: trim_steep == 0 is the hard gate of I3 (keep = d2 < trim2), > 0 the soft gate of I3'.  The mode is a
// launch constant, so the branch is uniform over the grid and the hard path is the arithmetic it always was.
template <int DIM, int TYPE>
__device__ __forceinline__ void point_terms(PointTerms<DIM, TYPE> &t, const float *T, const float *srow,
                                            const float *trow, float omega, int loss, float k, float k2,
                                            float trim2, float trim_dist, float trim_steep)
{
    constexpr int P = PointTerms<DIM, TYPE>::P;
    constexpr int NR = PointTerms<DIM, TYPE>::NR;
    t.s[0] = srow[0];
    t.s[1] = srow[1];
    t.s[2] = srow[2];
    transform_point<DIM>(T, t.s, t.p);
#pragma unroll
    for (int c = 0; c < DIM; ++c) t.ev[c] = trow[c] - t.p[c];
    float d2 = t.ev[0] * t.ev[0] + t.ev[1] * t.ev[1];
    if constexpr (DIM == 3) d2 = d2 + t.ev[2] * t.ev[2];
    t.d2 = d2;
    if (trim_steep > 0.f) {
        const float d = sqrtf(d2);
        const float th = tanhf(trim_steep * (d - trim_dist));
        t.d = d;
        t.th = th;
        t.keep = 0.5f - 0.5f * th;
    } else {
        t.d = 0.f;
        t.th = 0.f;
        t.keep = (d2 < trim2) ? 1.f : 0.f;
    }
    if (TYPE == MMK_ICP_PT2PL) {
#pragma unroll
        for (int c = 0; c < DIM; ++c) t.n[c] = trow[3 + c];
        float e = t.n[0] * t.ev[0] + t.n[1] * t.ev[1];
        if constexpr (DIM == 3) e = e + t.n[2] * t.ev[2];
        t.er[0] = e;
        t.r2 = e * e;
        if (DIM == 2) {
            t.J[0][0] = t.n[0];
            t.J[0][1] = t.n[1];
            t.J[0][2] = t.n[1] * t.p[0] - t.n[0] * t.p[1];
        } else {
            t.J[0][0] = t.n[0];
            t.J[0][1] = t.n[1];
            t.J[0][2] = t.n[DIM - 1];
            t.J[0][P - 3] = t.p[1] * t.n[DIM - 1] - t.p[DIM - 1] * t.n[1];
            t.J[0][P - 2] = t.p[DIM - 1] * t.n[0] - t.p[0] * t.n[DIM - 1];
            t.J[0][P - 1] = t.p[0] * t.n[1] - t.p[1] * t.n[0];
        }
    } else {
        t.r2 = d2;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            t.er[r] = t.ev[r];
#pragma unroll
            for (int c = 0; c < P; ++c) t.J[r][c] = 0.f;
            t.J[r][r] = 1.f;
        }
        if (DIM == 2) {
            t.J[0][2] = -t.p[1];
            t.J[NR - 1][2] = t.p[0];
        } else {
            const float px = t.p[0], py = t.p[1], pz = t.p[DIM - 1];
            t.J[0][P - 2] = pz;
            t.J[0][P - 1] = -py;
            t.J[1 % NR][P - 3] = -pz;
            t.J[1 % NR][P - 1] = px;
            t.J[2 % NR][P - 3] = py;
            t.J[2 % NR][P - 2] = -px;
        }
    }
    float rho = 1.f;
    if (loss == MMK_LOSS_CAUCHY) {
        rho = 1.0f / (1.0f + t.r2 / k2);
    } else if (loss == MMK_LOSS_HUBER) {
        const float r = sqrtf(t.r2);
        rho = (r <= k) ? 1.f : k / r;
    } else if (loss == MMK_LOSS_GEMAN_MCCLURE) {
        const float c = 1.0f / (1.0f + t.r2 / k2);      // Cauchy's expression
        rho = c * c;
    } else if (loss == MMK_LOSS_WELSCH) {
        rho = expf(-(t.r2 / k2));
    }
    t.rho = rho;
    t.omega = omega;
    t.w = (omega * t.keep) * rho;
}

// I3'': the pair's robust scale, trim distance and steepness from the device array `hyper` (rows of (k, trim_dist,
// trim_steep), row stride `hstride` = 0 shared | 3 per pair).  b is blockIdx.y, so the loads are uniform over the block.
// k2 and trim2 are the single fp32 products the host forms for the scalar launches.  The gate's MODE stays the launch
// constant (trim_steep 0 | > 0); in hard mode column 2 is never read.
struct HyperVals {
    float k, k2, trim2, trim_dist, trim_steep;
};

__device__ __forceinline__ HyperVals load_hyper(const float *__restrict__ hyper, int hstride, int b, float trim_steep_mode)
{
    const float *h = hyper + (size_t)b * hstride;
    HyperVals v;
    v.k = h[0];
    v.k2 = v.k * v.k;
    v.trim_dist = h[1];
    v.trim2 = v.trim_dist * v.trim_dist;
    v.trim_steep = trim_steep_mode > 0.f ? h[2] : 0.f;
    return v;
}

// A value of `hyper` the launch will use that is non-finite or out of range (k > 0 under a robust loss, trim_dist >= 0,
// steepness > 0 in soft mode): MMK_ICP_STATUS_BAD_HYPER.  (NaN fails every comparison.)
__device__ __forceinline__ bool hyper_is_bad(const HyperVals &v, int loss, bool soft)
{
    const float big = 3.4028234663852886e38f;
    bool ok = v.trim_dist >= 0.f && v.trim_dist <= big;
    if (loss != MMK_LOSS_NONE) ok = ok && v.k > 0.f && v.k <= big;
    if (soft) ok = ok && v.trim_steep > 0.f && v.trim_steep <= big;
    return !ok;
}

// I3''' (DESIGN.md §3): the soft correspondent.  `nb` are the point's k neighbours in key order (I2'), p its transformed
// position, temp the temperature tau (a squared length).  Per slot j, fp32, every operation rounded on its own:
//      d_j = nn_dist(row_j, p) (I2's expression, recomputed from the row);  e_j = expf(-(d_j - d_0) / tau);
//      S = sum_j e_j in slot order;  a_j = e_j / S.
// Nothing is stored per slot: k is a run-time loop bound, a per-lane array indexed by j would live in scratch memory, so
// each loop loads its row again (k rows of one point: L1 / L2 hits) and recomputes a_j.
// I3⁗ / I7⁗ (the _soft_t entries): with `tptr` the pair's tau is tptr[b * tstride] (tstride 0 shared | 1 per pair), read
// once per block -- b is blockIdx.y, the load is uniform -- and `temp` is not looked at; the expressions below are the same,
// so an array that holds a number call's fp32 value gives that call's bits.
struct SoftArgs {
    const unsigned long long *keys;      // (B,N,k) of grid_knn_kernel (the forward only)
    int k;
    float temp;
    const float *tptr = nullptr;         // (1 | B) device tau; NULL: `temp`
    int tstride = 0;
    int tcheck = 0;                      // the forward's first iteration: one thread per pair validates tau_b
    double *tparts = nullptr;            // the backward: (B,nblk) block partials of tau-bar for this iteration, or NULL
};

__device__ __forceinline__ float soft_temp(const SoftArgs &soft, int b)
{
    return soft.tptr != nullptr ? soft.tptr[(size_t)b * soft.tstride] : soft.temp;
}

// A device tau that is non-finite or <= 0: MMK_ICP_STATUS_BAD_HYPER.  (NaN fails every comparison.)
__device__ __forceinline__ bool soft_temp_is_bad(float tau) { return !(tau > 0.f && tau <= 3.4028234663852886e38f); }

template <int DIM>
__device__ __forceinline__ float soft_e(const float *row, const float p[DIM], float d0, float temp)
{
    const float d = nn_dist<DIM>(row[0], row[1], DIM == 3 ? row[2] : 0.f, p);
    return expf(-(d - d0) / temp);
}

template <int DIM>
__device__ __forceinline__ void soft_norm(const float *tgtb, int tgt_cols, const int32_t *nb, int k, const float p[DIM],
                                          float temp, float &d0, float &S)
{
    const float *r0 = tgtb + (size_t)nb[0] * tgt_cols;
    d0 = nn_dist<DIM>(r0[0], r0[1], DIM == 3 ? r0[2] : 0.f, p);
    S = 0.f;
    for (int j = 0; j < k; ++j) {
        const float e = soft_e<DIM>(tgtb + (size_t)nb[j] * tgt_cols, p, d0, temp);
        S = j == 0 ? e : S + e;
    }
}

// The virtual target row vr[6] = sum_j a_j row_j in slot order (xyz; for pt2pl the normal too, NOT renormalised: the row
// stays linear in a), each product and each sum rounded; it takes the target row's place in point_terms.
template <int DIM, int TYPE>
__device__ __forceinline__ void soft_virtual_row(const float *tgtb, int tgt_cols, const int32_t *nb, int k, const float p[DIM],
                                                 float temp, float d0, float S, float vr[6])
{
#pragma unroll
    for (int c = 0; c < 6; ++c) vr[c] = 0.f;
    for (int j = 0; j < k; ++j) {
        const float *row = tgtb + (size_t)nb[j] * tgt_cols;
        const float a = soft_e<DIM>(row, p, d0, temp) / S;
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
            const float v = a * row[c];
            vr[c] = j == 0 ? v : vr[c] + v;
            if constexpr (TYPE == MMK_ICP_PT2PL) {
                const float vn = a * row[3 + c];
                vr[3 + c] = j == 0 ? vn : vr[3 + c] + vn;
            }
        }
    }
}

// Accumulate A (upper triangle, row-major) and b for one pair; one point per thread.
// HP: k, trim_dist and the steepness come from `hyper` (I3'') instead of the launch's scalars; `hcheck` != 0 (the first
// iteration of a call) has one thread per pair validate them.
// SOFT (mmk_icp_forward_soft, I3'''): the point's k keys come from soft.keys, idx_out is (B,N,k), and the virtual row takes
// the correspondent's place; `packed` and the zero-row bookkeeping are not used.  SOFT = false is the kernel it always was.
// With soft.tptr (mmk_icp_forward_soft_t, I3⁗) tau is the pair's device value, and `soft.tcheck` != 0 (the first iteration
// of a call) has one thread per pair validate it.
template <int DIM, int TYPE, bool HP = false, bool SOFT = false>
__global__ __launch_bounds__(ACC_THREADS) void icp_accumulate_kernel(
    const float *__restrict__ src, const float *__restrict__ tgt, int tgt_cols,
    const float *__restrict__ weight, const float *__restrict__ Tk, const int32_t *__restrict__ active,
    const unsigned long long *__restrict__ packed, unsigned long long *__restrict__ packed_next,
    const int32_t *__restrict__ allzero, const int32_t *__restrict__ zrep, int nn_pts, int nn_nsb,
    int32_t *__restrict__ idx_out, int N, int M, int loss, float k,
    float k2, float trim2, float trim_dist, float trim_steep, double *__restrict__ partials, int32_t *__restrict__ status,
    const float *__restrict__ hyper, int hstride, int hcheck, SoftArgs soft)
{
    constexpr int P = PointTerms<DIM, TYPE>::P;
    constexpr int NR = PointTerms<DIM, TYPE>::NR;
    constexpr int NACC = nacc(DIM);
    const int b = blockIdx.y;
    if (active != nullptr && active[b] == 0) return;
    if constexpr (HP) {
        const HyperVals hv = load_hyper(hyper, hstride, b, trim_steep);
        if (hcheck != 0 && blockIdx.x == 0 && threadIdx.x == 0 && status != nullptr && hyper_is_bad(hv, loss, trim_steep > 0.f))
            atomicOr(status, (int32_t)MMK_ICP_STATUS_BAD_HYPER);
        k = hv.k, k2 = hv.k2, trim2 = hv.trim2, trim_dist = hv.trim_dist, trim_steep = hv.trim_steep;
    }
    float stemp = 0.f;
    if constexpr (SOFT) {
        stemp = soft_temp(soft, b);
        if (soft.tcheck != 0 && blockIdx.x == 0 && threadIdx.x == 0 && status != nullptr && soft_temp_is_bad(stemp))
            atomicOr(status, (int32_t)MMK_ICP_STATUS_BAD_HYPER);
    }
    const int i = blockIdx.x * ACC_THREADS + threadIdx.x;
    double acc[NACC];
#pragma unroll
    for (int a = 0; a < NACC; ++a) acc[a] = 0.0;

    if (i < N) {
        float T[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) T[q] = Tk[(size_t)b * 16 + q];
        PointTerms<DIM, TYPE> t;
        if constexpr (SOFT) {
            // the k keys -> idx_out (B,N,k), guarded like the single key below; then the virtual row
            const unsigned long long *kp = soft.keys + ((size_t)b * N + i) * soft.k;
            int32_t *nb = idx_out + ((size_t)b * N + i) * soft.k;
            for (int j = 0; j < soft.k; ++j) {
                const unsigned long long key = kp[j];
                const unsigned jraw = (unsigned)(key & 0xffffffffull);
                if ((key == NN_KEY_INIT || jraw >= (unsigned)M) && status != nullptr) atomicOr(status, (int32_t)MMK_ICP_STATUS_UNARMED_KEY);
                nb[j] = (int)min(jraw, (unsigned)(M - 1));
            }
            const float *srow = src + ((size_t)b * N + i) * 3;
            const float s[3] = {srow[0], srow[1], srow[2]};
            float p[DIM], vr[6], d0, S;
            transform_point<DIM>(T, s, p);
            const float *tgtb = tgt + (size_t)b * M * tgt_cols;
            soft_norm<DIM>(tgtb, tgt_cols, nb, soft.k, p, stemp, d0, S);
            soft_virtual_row<DIM, TYPE>(tgtb, tgt_cols, nb, soft.k, p, stemp, d0, S, vr);
            const float omega = weight ? weight[(size_t)b * N + i] : 1.f;
            point_terms<DIM, TYPE>(t, T, srow, vr, omega, loss, k, k2, trim2, trim_dist, trim_steep);
        } else {
            // consume the NN key; arm the OTHER key buffer for the next iteration's atomic mins (two buffers: a row of a
            // skipped all-zero block reads the key of the pair's first zero row, which another workgroup owns)
            int isrc = i;
            if (allzero != nullptr && allzero[(size_t)b * nn_nsb + i / nn_pts] != 0 && zrep[b] < (i / nn_pts) * nn_pts) isrc = zrep[b];
            const unsigned long long key = packed[(size_t)b * N + isrc];
            if (packed_next != nullptr) packed_next[(size_t)b * N + i] = NN_KEY_INIT;
            // An index outside the target can only come from a key nobody armed (every NN engine writes each row's key: range 0
            // of the scan always does, also for non-finite points).  It must not become an address -- and it must not pass
            // silently as correspondence 0 either: the launch raises MMK_ICP_STATUS_UNARMED_KEY in the caller's status word
            // (mmk_icp_status; dICP/ICP.py turns it into an MmkError), then clamps so that the rest of the launch stays in bounds.
            const unsigned jraw = (unsigned)(key & 0xffffffffull);
            if ((key == NN_KEY_INIT || jraw >= (unsigned)M) && status != nullptr) atomicOr(status, (int32_t)MMK_ICP_STATUS_UNARMED_KEY);
            const int j = (int)min(jraw, (unsigned)(M - 1));
            idx_out[(size_t)b * N + i] = j;
            const float omega = weight ? weight[(size_t)b * N + i] : 1.f;
            point_terms<DIM, TYPE>(t, T, src + ((size_t)b * N + i) * 3, tgt + ((size_t)b * M + j) * tgt_cols, omega,
                                   loss, k, k2, trim2, trim_dist, trim_steep);
        }
        int a = 0;
#pragma unroll
        for (int m = 0; m < P; ++m) {
#pragma unroll
            for (int n = m; n < P; ++n) {
                double v = 0.0;
#pragma unroll
                for (int r = 0; r < NR; ++r) v += (double)(t.w * t.J[r][m]) * (double)t.J[r][n];
                acc[a++] = v;
            }
        }
#pragma unroll
        for (int m = 0; m < P; ++m) {
            double v = 0.0;
#pragma unroll
            for (int r = 0; r < NR; ++r) v += (double)(t.w * t.J[r][m]) * (double)t.er[r];
            acc[a++] = v;
        }
    }

    __shared__ double red[ACC_THREADS / 64][NACC];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
        double v = wave_sum(acc[a]);
        if (lane == 0) red[wv][a] = v;
    }
    __syncthreads();
    if (threadIdx.x < NACC) {
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < ACC_THREADS / 64; ++w) v += red[w][threadIdx.x];
        partials[((size_t)b * gridDim.x + blockIdx.x) * NACC + threadIdx.x] = v;
    }
}

// ------------------------------------------------------------------------------------------
// Small dense fp64 helpers (one lane).
// (the callers keep A, rhs, x and the work space `ws` (P * P + P doubles) in LDS: as per-lane arrays with run-time indices
// they would live in scratch memory, which this library does not use anywhere -- see nn_mfma_kernel)
template <int P>
__device__ bool chol_solve(const double *A /*P*P row-major symmetric*/, const double *rhs, double *x, double *ws)
{
    double (*L)[P] = reinterpret_cast<double (*)[P]>(ws);
    double *y = ws + P * P;
    bool ok = true;
    for (int i = 0; i < P; ++i)
        for (int j = 0; j < P; ++j) {
            L[i][j] = 0.0;
            if (!isfinite(A[i * P + j])) ok = false;
        }
    for (int j = 0; j < P && ok; ++j) {
        double d = A[j * P + j];
        for (int q = 0; q < j; ++q) d -= L[j][q] * L[j][q];
        if (!(d > 0.0)) {
            ok = false;
            break;
        }
        d = sqrt(d);
        L[j][j] = d;
        for (int i = j + 1; i < P; ++i) {
            double v = A[i * P + j];
            for (int q = 0; q < j; ++q) v -= L[i][q] * L[j][q];
            L[i][j] = v / d;
        }
    }
    if (!ok) {
        for (int i = 0; i < P; ++i) x[i] = 0.0;
        return false;
    }
    for (int i = 0; i < P; ++i) {
        double v = rhs[i];
        for (int q = 0; q < i; ++q) v -= L[i][q] * y[q];
        y[i] = v / L[i][i];
    }
    for (int i = P - 1; i >= 0; --i) {
        double v = y[i];
        for (int q = i + 1; q < P; ++q) v -= L[q][i] * x[q];
        x[i] = v / L[i][i];
    }
    return true;
}

// Closed-form Exp(delta) -> 4x4 (oracle: se_exp).
template <int DIM>
__device__ void se_exp(const double *dl, double E[16])
{
    for (int i = 0; i < 16; ++i) E[i] = 0.0;
    E[0] = E[5] = E[10] = E[15] = 1.0;
    if (DIM == 2) {
        const double x = dl[0], y = dl[1], th = dl[2];
        const double th2 = th * th;
        double a, bb;
        if (th2 < 1e-8) {
            a = 1.0 - th2 / 6.0 + th2 * th2 / 120.0;
            bb = th * (0.5 - th2 / 24.0 + th2 * th2 / 720.0);
        } else {
            a = sin(th) / th;
            bb = (1.0 - cos(th)) / th;
        }
        const double c = cos(th), s = sin(th);
        E[0] = c; E[1] = -s; E[3] = a * x - bb * y;
        E[4] = s; E[5] = c;  E[7] = bb * x + a * y;
    } else {
        const double *rho = dl, *phi = dl + 3;
        const double th2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2];
        double A_, B_, C_;
        if (th2 < 1e-8) {
            A_ = 1.0 - th2 / 6.0 + th2 * th2 / 120.0;
            B_ = 0.5 - th2 / 24.0 + th2 * th2 / 720.0;
            C_ = 1.0 / 6.0 - th2 / 120.0 + th2 * th2 / 5040.0;
        } else {
            const double th = sqrt(th2);
            A_ = sin(th) / th;
            B_ = (1.0 - cos(th)) / th2;
            C_ = (th - sin(th)) / (th2 * th);
        }
        const double K[9] = {0.0, -phi[2], phi[1], phi[2], 0.0, -phi[0], -phi[1], phi[0], 0.0};
        double K2[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double v = 0.0;
                for (int q = 0; q < 3; ++q) v += K[i * 3 + q] * K[q * 3 + j];
                K2[i * 3 + j] = v;
            }
        for (int i = 0; i < 3; ++i) {
            double tv = 0.0;
            for (int j = 0; j < 3; ++j) {
                const double id = (i == j) ? 1.0 : 0.0;
                E[i * 4 + j] = id + A_ * K[i * 3 + j] + B_ * K2[i * 3 + j];
                tv += (id + B_ * K[i * 3 + j] + C_ * K2[i * 3 + j]) * rho[j];
            }
            E[i * 4 + 3] = tv;
        }
    }
}

// I5 + I6: sum the block partials in a fixed order, solve, update the pose.
template <int DIM>
__global__ __launch_bounds__(64) void icp_solve_kernel(const double *__restrict__ partials, int nblk,
                                                       const float *__restrict__ T_in, float *__restrict__ T_out,
                                                       double *__restrict__ delta_out, double *__restrict__ A_out,
                                                       const int32_t *__restrict__ active_in,
                                                       int32_t *__restrict__ active_out, float tol)
{
    constexpr int P = (DIM == 2) ? 3 : 6;
    constexpr int NACC = nacc(DIM);
    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    __shared__ double acc[NACC];
    __shared__ double stage[PART_ROWS * NACC];
    const bool act = active_in[b] != 0;
    {
        // the block partials, summed in index order as before; the wave fetches PART_ROWS rows at a time
        // (coalesced, all in flight) instead of one dependent load per row and lane
        double v = 0.0;
        if (act) {
            const double *base = partials + (size_t)b * nblk * NACC;
            for (int r0 = 0; r0 < nblk; r0 += PART_ROWS) {
                const int nr = min(PART_ROWS, nblk - r0);
                for (int e = lane; e < nr * NACC; e += 64) stage[e] = base[(size_t)r0 * NACC + e];
                __syncthreads();
                if (lane < NACC)
                    for (int q = 0; q < nr; ++q) v += stage[q * NACC + lane];
                __syncthreads();
            }
        }
        if (lane < NACC) acc[lane] = v;
    }
    __syncthreads();
    if (lane != 0) return;
    __shared__ double A[P * P], rhs[P], dl[6], E[16], ws[P * P + P];
    for (int q = 0; q < 6; ++q) dl[q] = 0.0;
    int a = 0;
    for (int m = 0; m < P; ++m)
        for (int n = m; n < P; ++n) {
            A[m * P + n] = acc[a];
            A[n * P + m] = acc[a];
            ++a;
        }
    for (int m = 0; m < P; ++m) rhs[m] = acc[a++];
    for (int q = 0; q < 36; ++q) A_out[(size_t)b * 36 + q] = (q < P * P) ? A[q] : 0.0;
    if (act) chol_solve<P>(A, rhs, dl, ws);
    for (int q = 0; q < 6; ++q) delta_out[(size_t)b * 6 + q] = dl[q];
    if (!act) {
        for (int q = 0; q < 16; ++q) T_out[(size_t)b * 16 + q] = T_in[(size_t)b * 16 + q];
        active_out[b] = 0;
        return;
    }
    se_exp<DIM>(dl, E);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double v = 0.0;
            for (int q = 0; q < 4; ++q) v += E[i * 4 + q] * (double)T_in[(size_t)b * 16 + q * 4 + j];
            T_out[(size_t)b * 16 + i * 4 + j] = (float)v;
        }
    double nrm = 0.0;
    for (int q = 0; q < P; ++q) nrm += dl[q] * dl[q];
    active_out[b] = (sqrt(nrm) < (double)tol) ? 0 : 1;
}

// The head of a forward call in ONE launch: nearest-neighbour keys armed (both buffers), status word cleared, every pair
// active, T_hist[0] = T_init, the zero-row representatives reset -- five copy / fill launches of 3-6 us each before.
__global__ __launch_bounds__(256) void icp_init_kernel(unsigned long long *__restrict__ keys, size_t nkeys, int32_t *__restrict__ status,
                                                       int32_t *__restrict__ active0, const float *__restrict__ T_init,
                                                       float *__restrict__ T0, int32_t *__restrict__ zrep, int B, int N)
{
    const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = i0; i < nkeys; i += stride) keys[i] = ~0ull;
    if (i0 < 16) status[i0] = 0;
    if (i0 < (size_t)B) {
        active0[i0] = 1;
        if (zrep != nullptr) zrep[i0] = N;
    }
    if (i0 < (size_t)B * 16) T0[i0] = T_init[i0];
}

__global__ void fill_i32_kernel(int32_t *p, int n, int32_t v)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// ------------------------------------------------------------------------------------------
// I7 backward, per-pair part.  One wave per pair; the 64 lanes are the 8x8 entries of the
// block matrix [[X^T, Ebar],[0, X^T]] whose exponential carries exp(X)^T (top-left) and the
// adjoint of the exponential map applied to Ebar (top-right).
template <int DIM>
__global__ __launch_bounds__(64) void icp_bwd_pair_kernel(
    const double *__restrict__ Gdir_in, const double *__restrict__ pparts, int nparts,
    const float *__restrict__ Tk, const double *__restrict__ delta, const double *__restrict__ Amat,
    const int32_t *__restrict__ active, double *__restrict__ Gdir_out, double *__restrict__ lam_out)
{
    constexpr int P = (DIM == 2) ? 3 : 6;
    constexpr int NP = npose(DIM);
    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    __shared__ double G[16], Eb[16], X[16], M0[64], R0[64], R1[64];
    __shared__ double stage[PART_ROWS * NP];

    // full gradient w.r.t. T_{k+1}: direct part + point path of the later iteration (the parts are
    // added in index order; rows are fetched PART_ROWS at a time by the whole wave)
    {
        double v = (lane < 16) ? Gdir_in[(size_t)b * 16 + lane] : 0.0;
        const int r = lane >> 2, c = lane & 3;
        int slot = -1;
        if (lane < 16 && r < DIM && c < DIM) slot = r * DIM + c;
        if (lane < 16 && r < DIM && c == 3) slot = DIM * DIM + r;
        const double *base = pparts + (size_t)b * nparts * NP;
        for (int r0 = 0; r0 < nparts; r0 += PART_ROWS) {
            const int nr = min(PART_ROWS, nparts - r0);
            for (int e = lane; e < nr * NP; e += 64) stage[e] = base[(size_t)r0 * NP + e];
            __syncthreads();
            if (slot >= 0)
                for (int q = 0; q < nr; ++q) v += stage[q * NP + slot];
            __syncthreads();
        }
        if (lane < 16) G[lane] = v;
    }
    __syncthreads();
    const bool act = (active != nullptr) && active[b] != 0;
    if (!act) {
        if (lane < 16) Gdir_out[(size_t)b * 16 + lane] = G[lane];
        if (lane < 6 && lam_out) lam_out[(size_t)b * 6 + lane] = 0.0;
        return;
    }
    const double *dl = delta + (size_t)b * 6;
    if (lane < 16) {
        const int r = lane >> 2, c = lane & 3;
        // Ebar = G * T_k^T
        double v = 0.0;
        for (int q = 0; q < 4; ++q) v += G[r * 4 + q] * (double)Tk[(size_t)b * 16 + c * 4 + q];
        Eb[lane] = v;
        double x = 0.0;
        if (DIM == 2) {
            if (r == 0 && c == 3) x = dl[0];
            if (r == 1 && c == 3) x = dl[1];
            if (r == 1 && c == 0) x = dl[2];
            if (r == 0 && c == 1) x = -dl[2];
        } else {
            if (c == 3 && r < 3) x = dl[r];
            if (r == 2 && c == 1) x = dl[3];
            if (r == 1 && c == 2) x = -dl[3];
            if (r == 0 && c == 2) x = dl[4];
            if (r == 2 && c == 0) x = -dl[4];
            if (r == 1 && c == 0) x = dl[5];
            if (r == 0 && c == 1) x = -dl[5];
        }
        X[lane] = x;
    }
    __syncthreads();
    const int i8 = lane >> 3, j8 = lane & 7;
    {
        double m = 0.0;
        const double sc = 1.0 / 64.0;
        if (i8 < 4 && j8 < 4) m = X[j8 * 4 + i8] * sc;             // X^T
        else if (i8 >= 4 && j8 >= 4) m = X[(j8 - 4) * 4 + (i8 - 4)] * sc;
        else if (i8 < 4 && j8 >= 4) m = Eb[i8 * 4 + (j8 - 4)] * sc;
        M0[lane] = m;
        R0[lane] = ((i8 == j8) ? 1.0 : 0.0) + m / 13.0;
    }
    __syncthreads();
    double *cur = R0, *nxt = R1;
    // Horner: R = I + M R / n, n = 12 .. 1
    for (int n = 12; n >= 1; --n) {
        double v = 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) v += M0[i8 * 8 + q] * cur[q * 8 + j8];
        nxt[lane] = ((i8 == j8) ? 1.0 : 0.0) + v / (double)n;
        __syncthreads();
        double *t = cur; cur = nxt; nxt = t;
    }
    for (int sq = 0; sq < 6; ++sq) {
        double v = 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) v += cur[i8 * 8 + q] * cur[q * 8 + j8];
        nxt[lane] = v;
        __syncthreads();
        double *t = cur; cur = nxt; nxt = t;
    }
    // cur = [[E^T, Xbar],[0, E^T]]
    if (lane < 16) {
        const int r = lane >> 2, c = lane & 3;
        double v = 0.0;
        for (int q = 0; q < 4; ++q) v += cur[r * 8 + q] * G[q * 4 + c];  // E^T G
        Gdir_out[(size_t)b * 16 + lane] = v;
    }
    if (lane == 0) {
        auto xb = [&](int r, int c) { return cur[r * 8 + 4 + c]; };
        __shared__ double db[P], A[P * P], lam[P], ws[P * P + P];
        if (DIM == 2) {
            db[0] = xb(0, 3);
            db[1] = xb(1, 3);
            db[2] = xb(1, 0) - xb(0, 1);
        } else {
            db[0] = xb(0, 3);
            db[1] = xb(1, 3);
            db[2] = xb(2, 3);
            db[P - 3] = xb(2, 1) - xb(1, 2);
            db[P - 2] = xb(0, 2) - xb(2, 0);
            db[P - 1] = xb(1, 0) - xb(0, 1);
        }
        for (int q = 0; q < P * P; ++q) A[q] = Amat[(size_t)b * 36 + q];
        // forward took delta = 0 when A was not positive definite: no dependence then
        chol_solve<P>(A, db, lam, ws);
        for (int q = 0; q < 6; ++q) lam_out[(size_t)b * 6 + q] = (q < P) ? lam[q] : 0.0;
    }
}

// Columns of a point's contribution row to the target gradient (PTS): q̄ (dim), then n̄ (dim) for pt2pl; and the columns of
// their fixed-point sums, padded to a power of two (icp_bwd_target_scatter_kernel).
__host__ __device__ constexpr int tgt_row_cols(int dim, int type) { return type == MMK_ICP_PT2PL ? 2 * dim : dim; }
__host__ __device__ constexpr int tgt_acc_cols(int c) { return c <= 2 ? 2 : (c <= 4 ? 4 : 8); }

// The adjoint of the target row a point read (I7): q̄ (dim), then n̄ (dim) for pt2pl, the soft gate's path gev included.
template <int DIM, int TYPE>
__device__ __forceinline__ void target_row_adjoint(const PointTerms<DIM, TYPE> &t, const float *ebar,
                                                   const float (*Jbar)[PointTerms<DIM, TYPE>::P], const float *gev,
                                                   float trim_steep, float *q)
{
    constexpr int P = PointTerms<DIM, TYPE>::P;
    if constexpr (TYPE == MMK_ICP_PT2PT) {
#pragma unroll
        for (int c = 0; c < DIM; ++c) q[c] = ebar[c];               // e = q − p
    } else {
        const float eb = ebar[0];                                   // e = n·(q − p), J = nᵀG
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
            q[c] = t.n[c] * eb;
            q[DIM + c] = eb * t.ev[c] + Jbar[0][c];
        }
        if constexpr (DIM == 2) {        // J[2] = ny·px − nx·py
            q[DIM + 0] -= t.p[1] * Jbar[0][2];
            q[DIM + 1] += t.p[0] * Jbar[0][2];
        } else {                         // J[3:6] = p × n: n̄ += J̄rot × p (as p̄ += n × J̄rot above)
            const float px = t.p[0], py = t.p[1], pz = t.p[DIM - 1];
            const float j3 = Jbar[0][P - 3], j4 = Jbar[0][P - 2], j5 = Jbar[0][P - 1];
            q[DIM + 0] += j4 * pz - j5 * py;
            q[DIM + 1] += j5 * px - j3 * pz;
            q[DIM + DIM - 1] += j3 * py - j4 * px;
        }
    }
    if (trim_steep > 0.f) {     // the gate's path into the correspondent's xyz (the normals get nothing from it)
#pragma unroll
        for (int c = 0; c < DIM; ++c) q[c] += gev[c];
    }
}

// I7 backward, per-point part: dL/dweight and the point path of dL/dT_k.
// PTS (mmk_icp_backward_points): also the adjoints of the clouds -- gsrc (B,N,3, may be NULL) += R_kᵀ p̄ in place (each
// thread owns its point, iterations are ordered launches), and the point's contribution to its correspondent's target
// gradient as a row of `rows` ((B,N,tgt_row_cols), may be NULL), with the pair's largest |entry| as float bits in pmax (B)
// by an INTEGER max (order independent): icp_bwd_target_scatter_kernel adds the rows up after the sweep.
// HP (mmk_icp_backward_hp, I7''): k, trim_dist and the steepness come from `hyper` as in the forward, and the block's fp64
// sums of the per-point adjoints (k̄, c̄, s̄) go to `hparts` (nblk,B rows of 3 for this iteration) by the reduction of the pose
// parts: wave shuffle -> LDS -> one partial per block, no atomics.  A frozen pair's blocks write exact zeros.
// SOFT (mmk_icp_backward_soft, I7'''): idx is (B,N,k), the virtual row is rebuilt as in the forward, the per-point code below
// yields its adjoint, and a last loop over the slots turns that into the k target rows (`rows` is (B,N*k,C)) and the
// softmin's share of p̄.  SOFT = false is the kernel it always was.  With soft.tparts (mmk_icp_backward_soft_t with
// grad_temp, I7⁗) the second slot loop also forms u = sum_j z̄_j (d_j - d_0), the point's tau-bar = u / (tau_b tau_b) goes
// through the reduction of the pose parts as one more fp64 accumulator, and the block's sum lands in soft.tparts (B,nblk);
// a frozen pair's blocks write exact zeros.  Without it that accumulator is neither summed nor stored.
template <int DIM, int TYPE, bool PTS, bool HP = false, bool SOFT = false>
__global__ __launch_bounds__(ACC_THREADS) void icp_bwd_point_kernel(
    const float *__restrict__ src, const float *__restrict__ tgt, int tgt_cols,
    const float *__restrict__ weight, const float *__restrict__ Tk, const int32_t *__restrict__ active,
    const int32_t *__restrict__ idx, const double *__restrict__ lam64, const double *__restrict__ delta64, int N,
    int M, int loss, float k, float k2, float trim2, float trim_dist, float trim_steep, float *__restrict__ gw,
    double *__restrict__ pparts,
    float *__restrict__ gsrc, float *__restrict__ rows, unsigned *__restrict__ pmax,
    const float *__restrict__ hyper, int hstride, double *__restrict__ hparts, SoftArgs soft)
{
    constexpr int P = PointTerms<DIM, TYPE>::P;
    constexpr int NR = PointTerms<DIM, TYPE>::NR;
    constexpr int NP = npose(DIM);
    constexpr int NH = HP ? 3 : (SOFT ? 1 : 0);     // SOFT: tau-bar (I7⁗), summed only when soft.tparts is given
    constexpr int C = tgt_row_cols(DIM, TYPE);
    const int b = blockIdx.y;
    const int i = blockIdx.x * ACC_THREADS + threadIdx.x;
    double acc[NP + NH];
#pragma unroll
    for (int a = 0; a < NP + NH; ++a) acc[a] = 0.0;
    if constexpr (HP) {
        const HyperVals hv = load_hyper(hyper, hstride, b, trim_steep);
        k = hv.k, k2 = hv.k2, trim2 = hv.trim2, trim_dist = hv.trim_dist, trim_steep = hv.trim_steep;
    }
    const bool act = active[b] != 0;
    unsigned mbits = 0u;
    float stemp = 0.f;
    if constexpr (SOFT) stemp = soft_temp(soft, b);

    if (act && i < N) {
        float T[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) T[q] = Tk[(size_t)b * 16 + q];
        float lam[P], dl[P];
#pragma unroll
        for (int q = 0; q < P; ++q) {
            lam[q] = (float)lam64[(size_t)b * 6 + q];
            dl[q] = (float)delta64[(size_t)b * 6 + q];
        }
        int j = 0;
        if constexpr (!SOFT) j = idx[(size_t)b * N + i];
        const float omega = weight ? weight[(size_t)b * N + i] : 1.f;
        PointTerms<DIM, TYPE> t;
        float sd0 = 0.f, sS = 1.f;           // SOFT: d_0 and S of the point
        if constexpr (SOFT) {
            const float *srow = src + ((size_t)b * N + i) * 3;
            const float s[3] = {srow[0], srow[1], srow[2]};
            float p[DIM], vr[6];
            transform_point<DIM>(T, s, p);
            const float *tgtb = tgt + (size_t)b * M * tgt_cols;
            const int32_t *nb = idx + ((size_t)b * N + i) * soft.k;
            soft_norm<DIM>(tgtb, tgt_cols, nb, soft.k, p, stemp, sd0, sS);
            soft_virtual_row<DIM, TYPE>(tgtb, tgt_cols, nb, soft.k, p, stemp, sd0, sS, vr);
            point_terms<DIM, TYPE>(t, T, srow, vr, omega, loss, k, k2, trim2, trim_dist, trim_steep);
        } else {
            point_terms<DIM, TYPE>(t, T, src + ((size_t)b * N + i) * 3, tgt + ((size_t)b * M + j) * tgt_cols, omega,
                                   loss, k, k2, trim2, trim_dist, trim_steep);
        }
        float wbar = 0.f;
        float ebar[NR];
        float Jbar[NR][P];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            float u = 0.f, v = 0.f;
#pragma unroll
            for (int c = 0; c < P; ++c) {
                u += t.J[r][c] * lam[c];
                v += t.J[r][c] * dl[c];
            }
            const float res = t.er[r] - v;
            wbar += u * res;
            ebar[r] = t.w * u;
#pragma unroll
            for (int c = 0; c < P; ++c) Jbar[r][c] = t.w * (res * lam[c] - u * dl[c]);
        }
        // w = (omega*keep)*rho
        const float gomega = wbar * t.keep * t.rho;
        const float rhobar = wbar * t.omega * t.keep;
        float r2bar = 0.f;
        if (loss == MMK_LOSS_CAUCHY) {
            r2bar = rhobar * (-(t.rho * t.rho) / k2);
        } else if (loss == MMK_LOSS_HUBER) {
            if (sqrtf(t.r2) > k) r2bar = rhobar * (-t.rho / (2.f * t.r2));
        } else if (loss == MMK_LOSS_GEMAN_MCCLURE) {    // rho = c c: c by the forward's expression
            const float c = 1.0f / (1.0f + t.r2 / k2);
            r2bar = rhobar * (-(2.f * (c * t.rho)) / k2);
        } else if (loss == MMK_LOSS_WELSCH) {
            r2bar = rhobar * (-t.rho / k2);
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) ebar[r] += 2.f * t.er[r] * r2bar;
        gw[(size_t)b * N + i] += gomega;
        if constexpr (HP) {             // k̄ (I7''): rho = 1 / (1 + r2 / k2) | k / r past the knee | c c | exp(-(r2 / k2))
            float kbar = 0.f;
            if (loss == MMK_LOSS_CAUCHY) {
                kbar = rhobar * ((2.f * t.r2 * (t.rho * t.rho)) / (k * k2));
            } else if (loss == MMK_LOSS_HUBER) {
                const float r = sqrtf(t.r2);
                if (r > k) kbar = rhobar / r;
            } else if (loss == MMK_LOSS_GEMAN_MCCLURE) {
                const float c = 1.0f / (1.0f + t.r2 / k2);
                kbar = rhobar * ((4.f * t.r2 * (c * t.rho)) / (k * k2));
            } else if (loss == MMK_LOSS_WELSCH) {
                kbar = rhobar * ((2.f * t.r2 * t.rho) / (k * k2));
            }
            acc[NP + 0] = (double)kbar;
        }

        float pbar[DIM];
#pragma unroll
        for (int c = 0; c < DIM; ++c) pbar[c] = 0.f;
        if (TYPE == MMK_ICP_PT2PT) {
#pragma unroll
            for (int c = 0; c < DIM; ++c) pbar[c] -= ebar[c % NR];
            if (DIM == 2) {
                pbar[1] -= Jbar[0][2];
                pbar[0] += Jbar[NR - 1][2];
            } else {
                pbar[DIM - 1] += Jbar[0][P - 2];
                pbar[1] -= Jbar[0][P - 1];
                pbar[DIM - 1] -= Jbar[1 % NR][P - 3];
                pbar[0] += Jbar[1 % NR][P - 1];
                pbar[1] += Jbar[2 % NR][P - 3];
                pbar[0] -= Jbar[2 % NR][P - 2];
            }
        } else {
#pragma unroll
            for (int c = 0; c < DIM; ++c) pbar[c] -= t.n[c] * ebar[0];
            if (DIM == 2) {
                pbar[0] += t.n[1] * Jbar[0][2];
                pbar[1] -= t.n[0] * Jbar[0][2];
            } else {
                const float nx = t.n[0], ny = t.n[1], nz = t.n[DIM - 1];
                const float j3 = Jbar[0][P - 3], j4 = Jbar[0][P - 2], j5 = Jbar[0][P - 1];
                pbar[0] += -nz * j4 + ny * j5;
                pbar[1] += nz * j3 - nx * j5;
                pbar[DIM - 1] += -ny * j3 + nx * j4;
            }
        }
        // soft gate (I7'): keep = 0.5 - 0.5 tanh(steep (d - trim)), d = |ev|, ev = q - p; a coincident point (d == 0) gets 0
        float gev[DIM];
#pragma unroll
        for (int c = 0; c < DIM; ++c) gev[c] = 0.f;
        if (trim_steep > 0.f) {
            const float keepbar = (wbar * t.omega) * t.rho;
            const float dbar = keepbar * (-0.5f * trim_steep * (1.f - t.th * t.th));
#pragma unroll
            for (int c = 0; c < DIM; ++c) {
                gev[c] = (t.d > 0.f) ? dbar * (t.ev[c] / t.d) : 0.f;
                pbar[c] -= gev[c];
            }
            if constexpr (HP) {         // c̄, s̄ (I7''): the hard gate is a constant and leaves both at exactly 0
                const float g = 0.5f * (1.f - t.th * t.th);
                acc[NP + 1] = (double)(keepbar * (trim_steep * g));
                acc[NP + 2] = (double)(keepbar * (-g * (t.d - trim_dist)));
            }
        }
        if constexpr (SOFT) {
            // I7''': q holds the adjoint of the virtual row [q̃̄ ; ñ̄].  Per slot ā_j = q̃̄·q_j (+ ñ̄·n_j); m = sum_l a_l ā_l in
            // slot order (first loop); then z̄_j = a_j (ā_j - m), d̄_j = -z̄_j / tau, the slot's target row a_j [q̃̄ ; ñ̄] with
            // 2 d̄_j (q_j - p) added to its xyz, and the same vector taken off p̄ (second loop).  Which rows are the
            // neighbours is a constant; tau gets its gradient from the same z̄_j when soft.tparts is given (I7⁗).
            float q[C];
            target_row_adjoint<DIM, TYPE>(t, ebar, Jbar, gev, trim_steep, q);
            const float *tgtb = tgt + (size_t)b * M * tgt_cols;
            const int32_t *nb = idx + ((size_t)b * N + i) * soft.k;
            auto abar = [&](const float *row) {
                float v = q[0] * row[0];
#pragma unroll
                for (int c = 1; c < DIM; ++c) v += q[c] * row[c];
                if constexpr (TYPE == MMK_ICP_PT2PL) {
#pragma unroll
                    for (int c = 0; c < DIM; ++c) v += q[DIM + c] * row[3 + c];
                }
                return v;
            };
            float m = 0.f, tu = 0.f;
            for (int j = 0; j < soft.k; ++j) {
                const float *row = tgtb + (size_t)nb[j] * tgt_cols;
                const float a = soft_e<DIM>(row, t.p, sd0, stemp) / sS;
                const float v = a * abar(row);
                m = j == 0 ? v : m + v;
            }
            for (int j = 0; j < soft.k; ++j) {
                const float *row = tgtb + (size_t)nb[j] * tgt_cols;
                const float a = soft_e<DIM>(row, t.p, sd0, stemp) / sS;
                const float zbar = a * (abar(row) - m);
                const float g = 2.f * (-zbar / stemp);
                if (soft.tparts != nullptr) {       // I7⁗: u = sum_j z̄_j (d_j - d_0) in slot order; slot 0 adds exactly 0
                    const float dj = nn_dist<DIM>(row[0], row[1], DIM == 3 ? row[2] : 0.f, t.p);
                    const float v = zbar * (dj - sd0);
                    tu = j == 0 ? v : tu + v;
                }
                float out[C];
#pragma unroll
                for (int c = 0; c < DIM; ++c) {
                    const float h = g * (row[c] - t.p[c]);
                    out[c] = a * q[c] + h;
                    pbar[c] -= h;
                    if constexpr (TYPE == MMK_ICP_PT2PL) out[DIM + c] = a * q[DIM + c];
                }
                if constexpr (PTS) {
                    if (rows != nullptr) {
                        float *orow = rows + (((size_t)b * N + i) * soft.k + j) * C;
#pragma unroll
                        for (int c = 0; c < C; ++c) {
                            orow[c] = out[c];
                            mbits = max(mbits, __float_as_uint(fabsf(out[c])));
                        }
                    }
                }
            }
            if (soft.tparts != nullptr) acc[NP] = (double)(tu / (stemp * stemp));
        }
        // p = R s + t
#pragma unroll
        for (int r = 0; r < DIM; ++r) {
#pragma unroll
            for (int c = 0; c < DIM; ++c) acc[r * DIM + c] = (double)pbar[r] * (double)t.s[c];
            acc[DIM * DIM + r] = (double)pbar[r];
        }
        if constexpr (PTS) {
            if (gsrc != nullptr) {          // s̄ += R_kᵀ p̄ (the DIM x DIM block of T_k); source z stays 0 in dim 2
                float *gs = gsrc + ((size_t)b * N + i) * 3;
#pragma unroll
                for (int c = 0; c < DIM; ++c) {
                    float v = T[c] * pbar[0];
#pragma unroll
                    for (int r = 1; r < DIM; ++r) v += T[r * 4 + c] * pbar[r];
                    gs[c] += v;
                }
            }
            if (!SOFT && rows != nullptr) {
                float q[C];                 // ∂L/∂(correspondent's xyz), then ∂L/∂(its normal) for pt2pl
                target_row_adjoint<DIM, TYPE>(t, ebar, Jbar, gev, trim_steep, q);
                float *row = rows + ((size_t)b * N + i) * C;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    row[c] = q[c];
                    mbits = max(mbits, __float_as_uint(fabsf(q[c])));      // (NaN patterns sort above +inf)
                }
            }
        }
    }

    __shared__ double red[ACC_THREADS / 64][NP + NH];
    __shared__ unsigned wmax[ACC_THREADS / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if constexpr (PTS) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mbits = max(mbits, __shfl_xor(mbits, off, 64));
        if (lane == 0) wmax[wv] = mbits;
    }
#pragma unroll
    for (int a = 0; a < NP + NH; ++a) {
        if (SOFT && a == NP && soft.tparts == nullptr) continue;        // (uniform over the grid)
        double v = wave_sum(acc[a]);
        if (lane == 0) red[wv][a] = v;
    }
    __syncthreads();
    if constexpr (PTS) {            // one integer max per block into the pair's word
        if (rows != nullptr && threadIdx.x == 0) {
            unsigned m = 0u;
#pragma unroll
            for (int w = 0; w < ACC_THREADS / 64; ++w) m = max(m, wmax[w]);
            if (m != 0u) atomicMax(&pmax[b], m);
        }
    }
    if (threadIdx.x < NP) {
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < ACC_THREADS / 64; ++w) v += red[w][threadIdx.x];
        pparts[((size_t)b * gridDim.x + blockIdx.x) * NP + threadIdx.x] = v;
    }
    if constexpr (HP) {
        if (threadIdx.x >= 64 && threadIdx.x < 64 + NH) {       // (a wave of its own: wave 0 writes the pose parts)
            const int c = threadIdx.x - 64;
            double v = 0.0;
#pragma unroll
            for (int w = 0; w < ACC_THREADS / 64; ++w) v += red[w][NP + c];
            hparts[((size_t)b * gridDim.x + blockIdx.x) * 3 + c] = v;
        }
    }
    if constexpr (SOFT) {
        if (soft.tparts != nullptr && threadIdx.x == 64) {          // (a wave of its own, as above)
            double v = 0.0;
#pragma unroll
            for (int w = 0; w < ACC_THREADS / 64; ++w) v += red[w][NP];
            soft.tparts[(size_t)b * gridDim.x + blockIdx.x] = v;
        }
    }
}

// grad_hyper (B,3) = the ordered sum of a pair's block partials over the iterations and blocks: `hparts` is (K,B,nblk,3).
// One wave per pair: lane l adds the rows l, l + 64, ... in index order, then the lanes are added by the fixed shuffle tree
// -- the same order in every run.  NC = 1: grad_temp (B) from the tau-bar partials (K,B,nblk) of the _soft_t entry (I7⁗).
template <int NC = 3>
__global__ __launch_bounds__(64) void icp_bwd_hyper_final_kernel(const double *__restrict__ hparts, int K, int B, int nblk,
                                                                 float *__restrict__ grad_hyper)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    double v[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) v[c] = 0.0;
    for (int e = lane; e < K * nblk; e += 64) {
        const int it = e / nblk, blk = e % nblk;
        const double *row = hparts + (((size_t)it * B + b) * nblk + blk) * NC;
#pragma unroll
        for (int c = 0; c < NC; ++c) v[c] += row[c];
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const double s = wave_sum(v[c]);
        if (lane == 0) grad_hyper[(size_t)b * NC + c] = (float)s;
    }
}

__global__ void f32_to_f64_kernel(const float *in, double *out, int n)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (double)in[i];
}

template <int DIM>
__global__ void bwd_final_kernel(const double *__restrict__ Gdir, const double *__restrict__ pparts, int nparts,
                                 float *__restrict__ out)
{
    constexpr int NP = npose(DIM);
    __shared__ double stage[PART_ROWS * NP];
    const int b = blockIdx.x, lane = threadIdx.x;
    double v = (lane < 16) ? Gdir[(size_t)b * 16 + lane] : 0.0;
    const int r = lane >> 2, c = lane & 3;
    int slot = -1;
    if (lane < 16 && r < DIM && c < DIM) slot = r * DIM + c;
    if (lane < 16 && r < DIM && c == 3) slot = DIM * DIM + r;
    const double *base = pparts + (size_t)b * nparts * NP;
    for (int r0 = 0; r0 < nparts; r0 += PART_ROWS) {
        const int nr = min(PART_ROWS, nparts - r0);
        for (int e = lane; e < nr * NP; e += blockDim.x) stage[e] = base[(size_t)r0 * NP + e];
        __syncthreads();
        if (slot >= 0)
            for (int q = 0; q < nr; ++q) v += stage[q * NP + slot];
        __syncthreads();
    }
    if (lane < 16) out[(size_t)b * 16 + lane] = (float)v;
}

// ------------------------------------------------------------------------------------------
// I7 backward, target gradient (mmk_icp_backward_points).  Up to K·N rows of a pair land on one target (every zero-padded
// source row maps to the same one), so the rows are added as FIXED POINT in 64-bit integers, whose sum does not depend on
// the order of arrival: entry v becomes llrint(v·scale), scale the power of two with K·N·max|v|·scale < 2^62 (no partial
// sum can overflow) -- a resolution of max|v|·2^(cnt_bits − 62) per entry, cnt_bits = ceil(log2(K·N)).  A non-finite entry
// (pmax bits >= +inf) makes the pair's target gradient NaN.  The scale is tgt_fixed_scale of mmk_common.h.

// One thread per (row, column), L = tgt_acc_cols(C) lanes per row, so that an atomic wave-instruction adds 64 / L whole rows
// (C·8 contiguous bytes each) instead of 64 scattered words.  A wave whose rows all share one target (the hot target) sums
// them first and adds once per column.  Rows of frozen pairs (never written) and zero entries (zero-weight rows) are skipped.
template <int C>
__global__ __launch_bounds__(ACC_THREADS) void icp_bwd_target_scatter_kernel(
    const float *__restrict__ rows, const int32_t *__restrict__ idx_hist, const int32_t *__restrict__ active_hist,
    const unsigned *__restrict__ pmax, int B, int N, int M, int cnt_bits, unsigned long long *__restrict__ acc)
{
    constexpr int L = tgt_acc_cols(C);
    const int b = blockIdx.y, k = blockIdx.z;
    const double scale = tgt_fixed_scale(pmax[b], cnt_bits);
    if (active_hist[(size_t)k * B + b] == 0 || scale == 0.0) return;       // (uniform over the block)
    const int t = blockIdx.x * ACC_THREADS + threadIdx.x, i = t / L, c = t % L;
    const bool valid = i < N;
    const size_t r = ((size_t)k * B + b) * N + i;
    const int j = valid ? idx_hist[r] : -1;
    long long v = 0;
    if (valid && c < C) v = llrint((double)rows[r * C + c] * scale);
    const unsigned long long vmask = __ballot(valid);
    if (vmask == 0ull) return;                                              // (uniform over the wave)
    unsigned long long *ab = acc + (size_t)b * M * L;
    const int j0 = __shfl(j, __ffsll(vmask) - 1, 64);
    if (__ballot(valid && j != j0) == 0ull) {
#pragma unroll
        for (int off = 32; off >= L; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((threadIdx.x & 63) < L && v != 0) atomicAdd(&ab[(size_t)j0 * L + c], (unsigned long long)v);
    } else if (v != 0) {
        atomicAdd(&ab[(size_t)j * L + c], (unsigned long long)v);
    }
}

// (B,M,L) fixed-point sums -> grad_target (B,M,cols): xyz columns < dim, pt2pl normal columns 3 .. 3 + dim; the rest 0.
__global__ void icp_bwd_target_final_kernel(const unsigned long long *__restrict__ acc, const unsigned *__restrict__ pmax,
                                            int cnt_bits, int M, int dim, int C, int L, int cols, float *__restrict__ gtgt)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (j >= M) return;
    const double scale = tgt_fixed_scale(pmax[b], cnt_bits);
    const unsigned long long *a = acc + ((size_t)b * M + j) * L;
    float *out = gtgt + ((size_t)b * M + j) * cols;
    for (int c = 0; c < cols; ++c) {
        const int e = c < dim ? c : (C > dim && c >= 3 && c < 3 + dim ? dim + (c - 3) : -1);
        float v = 0.f;
        if (e >= 0) v = scale == 0.0 ? __builtin_nanf("") : (float)((double)(long long)a[e] / scale);
        out[c] = v;
    }
}

// ------------------------------------------------------------------------------------------ host
// Run-time value -> template argument: f is called with a std::integral_constant per choice and instantiates the kernel.
template <class F>
auto with_bool(bool b, F &&f)
{
    return b ? f(std::true_type{}) : f(std::false_type{});
}

template <class F>
auto with_dim(int dim, F &&f)
{
    return dim == 2 ? f(std::integral_constant<int, 2>{}) : f(std::integral_constant<int, 3>{});
}

template <class F>
auto with_dim_type(int dim, int icp_type, F &&f)
{
    return with_dim(dim, [&](auto D) {
        return icp_type == MMK_ICP_PT2PT ? f(D, std::integral_constant<int, MMK_ICP_PT2PT>{})
                                         : f(D, std::integral_constant<int, MMK_ICP_PT2PL>{});
    });
}

template <class F>
auto with_bools(bool a, bool b, F &&f)
{
    return with_bool(a, [&](auto A) { return with_bool(b, [&](auto B) { return f(A, B); }); });
}

// Blocks of the per-point kernels (accumulate, backward sweep) per pair = rows of their block partials.
inline int acc_blocks(int N) { return (N + ACC_THREADS - 1) / ACC_THREADS; }

struct NNPlan {
    int Mpad, ntiles, nsb, ntu, tiles_per_unit, total_units, grid, P, ucap;
};

NNPlan nn_plan(int B, int N, int M, int dim)
{
    NNPlan pl;
    pl.P = 2;                                   // points per lane of the vector-pipe filter = 512-point source blocks for both kernels
    pl.Mpad = (int)mmk::align_up((size_t)M, NN_TILE);
    pl.ntiles = pl.Mpad / NN_TILE;
    pl.nsb = (N + NN_THREADS * pl.P - 1) / (NN_THREADS * pl.P);
    // Vector-pipe filter: single tiles -- short ranges balance the CUs better, and a range without candidates below the starting
    // bound costs no atomic (5 / 3 / 2 / 1 tiles per unit = 159 / 154 / 147 / 141 us per launch).  Matrix-core filter: a lane's
    // running bound restarts with every unit, and without a seed (the first ICP iteration) every restart flags a "record"
    // sequence of chunks that the exact part then re-scans: 324 / 170 us for the first / a later launch at 1 tile per unit,
    // 265 / 162 at 2, 226 / 157 at 4 (round-3 build before the last tuning; the final kernel: 314 / 148 at 1 tile, 257 / 143 at 2,
    // 195 / 133 at 4, 191 / 141 at 5, 210 / 163 at 10 -- each unit start costs two dependent gathers for the seed).
    pl.tiles_per_unit = std::min(4, pl.ntiles);
    pl.ntu = (pl.ntiles + pl.tiles_per_unit - 1) / pl.tiles_per_unit;
    const int Bpad = (B + 7) / 8 * 8;
    pl.total_units = Bpad * pl.nsb * pl.ntu;
    pl.ucap = (Bpad / 8) * pl.nsb;             // entries per class of the scanned-block lists (src_units_kernel)
    // persistent grid: 8 blocks of 256 threads per CU on the 256 CUs (LDS 8-12 KB, <= 64 VGPRs); 3 of the matrix-core
    // kernel's (40 KB of LDS each, <= 128 VGPRs)
    pl.grid = std::min(pl.total_units, dim == 2 ? 1024 : 768);
    return pl;
}

// Optional in-library timing of the NN kernel (bench.py's roofline leg): a pool of HIP
// event pairs recorded on the launch stream around each nn_search launch.
struct NNProf {
    bool on = false;
    int cap = 0, n = 0;
    hipEvent_t *ev = nullptr;  // 2 * cap
};
thread_local NNProf g_prof;      // per host thread: the library keeps no process-global mutable state

// `packed` (B,N) must hold NN_KEY_INIT on entry (memset 0xFF or re-armed by the accumulate kernel).
// `seed_buf` ((B,N) int32, may be null): where the coarse pass puts the seeds of a launch without previous correspondents.
int launch_nn(int dim, const float *src, const float *tgtp, const float *Tk, const int32_t *active,
              const int32_t *prev_idx, const int32_t *ulist, const int32_t *ucnt, int B, int N, const NNPlan &pl,
              unsigned long long *packed, int32_t *seed_buf, const int32_t *allzero, const int32_t *zrep, const float *dec,
              hipStream_t st)
{
    const bool rec = g_prof.on && g_prof.n < g_prof.cap;
    if (rec) MMK_CHECK_HIP(hipEventRecord(g_prof.ev[2 * g_prof.n], st));
    if (prev_idx == nullptr && seed_buf != nullptr && pl.Mpad >= 4 * NN_COARSE_STRIDE) {
        const dim3 grid((N + NN_COARSE_THREADS - 1) / NN_COARSE_THREADS, B);
        const int nn_pts = NN_THREADS * pl.P;
        with_dim(dim, [&](auto D) {
            hipLaunchKernelGGL(nn_coarse_seed_kernel<D()>, grid, dim3(NN_COARSE_THREADS), 0, st, src, tgtp, Tk, active, allzero, zrep, nn_pts,
                               pl.nsb, N, pl.Mpad, dec, seed_buf);
        });
        MMK_LAUNCH_CHECK();
        prev_idx = seed_buf;
    }
    constexpr float U = 5.9604645e-8f;       // 2^-24
    with_dim(dim, [&](auto D) {
        hipLaunchKernelGGL((nn_mfma_kernel<D()>), dim3(pl.grid), dim3(NN_THREADS), 0, st, src, tgtp, Tk, active, prev_idx, ulist, ucnt,
                           pl.ucap, B, N, pl.Mpad, pl.nsb, pl.ntu, pl.tiles_per_unit, pl.total_units, (D() == 2 ? 360.0f : 496.0f) * U,
                           packed);
    });
    MMK_LAUNCH_CHECK();
    if (rec) {
        MMK_CHECK_HIP(hipEventRecord(g_prof.ev[2 * g_prof.n + 1], st));
        g_prof.n++;
    }
    return MMK_OK;
}

int check_params(const mmk_icp_params *p)
{
    MMK_REQUIRE(p != nullptr, "mmk_icp: params is NULL");
    MMK_REQUIRE(p->B >= 1 && p->N >= 1 && p->M >= 1, "mmk_icp: B, N, M must be >= 1 (got %d, %d, %d)", p->B, p->N, p->M);
    MMK_REQUIRE(p->dim == 2 || p->dim == 3, "mmk_icp: dim must be 2 or 3 (got %d)", p->dim);
    MMK_REQUIRE(p->tgt_cols == 3 || p->tgt_cols == 6, "mmk_icp: target must have 3 or 6 columns (got %d)", p->tgt_cols);
    MMK_REQUIRE(p->icp_type == MMK_ICP_PT2PT || p->icp_type == MMK_ICP_PT2PL, "mmk_icp: bad icp_type %d", p->icp_type);
    MMK_REQUIRE(p->icp_type != MMK_ICP_PT2PL || p->tgt_cols == 6, "mmk_icp: pt2pl needs target normals (B,M,6)");
    MMK_REQUIRE(p->loss >= MMK_LOSS_NONE && p->loss <= MMK_LOSS_WELSCH, "mmk_icp: bad loss %d", p->loss);
    MMK_REQUIRE(p->max_iter >= 1, "mmk_icp: max_iter must be >= 1");
    MMK_REQUIRE(p->loss == MMK_LOSS_NONE || p->loss_k > 0.f, "mmk_icp: loss metric must be > 0");
    MMK_REQUIRE(p->nn_method == MMK_NN_BRUTE || p->nn_method == MMK_NN_GRID, "mmk_icp: bad nn_method %d", p->nn_method);
    MMK_REQUIRE(std::isfinite(p->trim_steep) && p->trim_steep >= 0.f, "mmk_icp: trim_steep must be finite and >= 0 (got %g)",
                (double)p->trim_steep);
    return MMK_OK;
}

// The robust-loss and trim arguments of the per-point kernels; k2 and trim2 are single fp32 products (I3).
struct RobustArgs {
    int loss;
    float k, k2, trim2, trim_dist, trim_steep;
};

RobustArgs robust_args(const mmk_icp_params *p)
{
    return {p->loss, p->loss_k, p->loss_k * p->loss_k, p->trim_dist * p->trim_dist, p->trim_dist, p->trim_steep};
}

struct IcpWs {
    float *tgtp;
    unsigned long long *packed;  // 2 x (B,N) NN keys: read by iteration k's accumulate, armed for iteration k+1
    int32_t *allzero, *zrep;     // (B,nsb), (B): zero-row bookkeeping of the source (src_zero_scan_kernel)
    int32_t *ulist, *ucnt;       // (8,ucap), (16): the source blocks the NN kernel scans (src_units_kernel)
    int32_t *seed0;              // (B,N): coarse seeds of the first iteration (nn_coarse_seed_kernel)
    float *tdec;                 // (B,dim,Mpad/NN_COARSE_STRIDE): every 64th target, densely (its samples)
    double *partials;   // forward: (B,nblk,NACC); backward: pose parts (B,nblk,NP)
    double *G0, *G1;    // backward (B,16)
    double *lam;        // backward (B,6)
    int32_t *status;             // (16): word 0 = MMK_ICP_STATUS_* bits raised by the kernels of the last forward call
    int32_t *g_counts, *g_cursor, *g_starts;  // grid NN: (B,NC), (B,NC), (B,NC+1)
    float4 *g_sorted;                          // grid NN: (B,M) x,y,z,index
    size_t bytes;
};

IcpWs carve(const mmk_icp_params *p, void *ws, size_t cap)
{
    const NNPlan pl = nn_plan(p->B, p->N, p->M, p->dim);
    const int nblk = acc_blocks(p->N);
    mmk::Arena ar(ws, cap);
    IcpWs w;
    w.tgtp = ar.take<float>((size_t)p->B * p->dim * pl.Mpad);
    w.packed = ar.take<unsigned long long>((size_t)2 * p->B * p->N);
    w.allzero = ar.take<int32_t>((size_t)p->B * pl.nsb);
    w.zrep = ar.take<int32_t>((size_t)p->B);
    w.ulist = ar.take<int32_t>((size_t)8 * pl.ucap);
    w.ucnt = ar.take<int32_t>(16);
    w.seed0 = ar.take<int32_t>((size_t)p->B * p->N);
    w.tdec = ar.take<float>((size_t)p->B * p->dim * (pl.Mpad / NN_COARSE_STRIDE));
    w.partials = ar.take<double>((size_t)p->B * nblk * 27);
    w.G0 = ar.take<double>((size_t)p->B * 16);
    w.G1 = ar.take<double>((size_t)p->B * 16);
    w.lam = ar.take<double>((size_t)p->B * 6);
    w.status = ar.take<int32_t>(16);
    w.g_counts = w.g_cursor = w.g_starts = nullptr;
    w.g_sorted = nullptr;
    if (p->nn_method == MMK_NN_GRID) {
        w.g_counts = ar.take<int32_t>((size_t)p->B * GRID_NC * 2);
        w.g_cursor = w.g_counts + (size_t)p->B * GRID_NC;
        w.g_starts = ar.take<int32_t>((size_t)p->B * (GRID_NC + 1));
        w.g_sorted = ar.take<float4>((size_t)p->B * p->M);
    }
    w.bytes = mmk::align_up(ar.off, 256);
    return w;
}

// Workspace of the backward entries, five parts in this order, each starting on a 256-byte boundary: the forward's
// (carve), the target gradient's (with_target), the hyper-parameter gradient's (with_hyper), the soft correspondences'
// (soft_k > 0; mmk_icp_forward_soft's workspace is the forward's part and this one), the temperature gradient's
// (with_temp).  A part that is not asked
// for takes no room and leaves its pointers NULL, so mmk_icp_backward's workspace is the forward's.
struct IcpBwdWs {
    IcpWs w;
    float *rows = nullptr;               // (K,B,N,C): every point's contribution row to the target gradient, per iteration
    unsigned long long *acc = nullptr;   // (B,M,L): their fixed-point sums
    unsigned *pmax = nullptr;            // (B): float bits of the largest |entry| of a pair's rows
    double *hparts = nullptr;            // (K,B,nblk,3): block partials of (k̄, c̄, s̄), every entry written by the sweep
    unsigned long long *soft_keys = nullptr;     // (B,N,k): the k-NN keys of the iteration in flight (soft correspondences)
    double *tparts = nullptr;            // (K,B,nblk): block partials of tau-bar (mmk_icp_backward_soft_t with grad_temp)
    size_t bytes = 0;
};

// soft_k > 0 (the _soft entries; p->nn_method is MMK_NN_GRID there): the target part holds k rows per point and the soft
// part, the last one, the keys of grid_knn_kernel.
IcpBwdWs carve_backward(const mmk_icp_params *p, bool with_target, bool with_hyper, void *ws, size_t cap, int soft_k = 0,
                        bool with_temp = false)
{
    IcpBwdWs b;
    b.w = carve(p, ws, cap);
    mmk::Arena ar(ws, cap);
    ar.off = b.w.bytes;
    if (with_target) {
        const int C = tgt_row_cols(p->dim, p->icp_type);
        b.rows = ar.take<float>((size_t)p->max_iter * p->B * p->N * std::max(soft_k, 1) * C);
        b.acc = ar.take<unsigned long long>((size_t)p->B * p->M * tgt_acc_cols(C));
        b.pmax = ar.take<unsigned>((size_t)p->B);
    }
    if (with_hyper) b.hparts = ar.take<double>((size_t)p->max_iter * p->B * acc_blocks(p->N) * 3);
    if (soft_k > 0) b.soft_keys = ar.take<unsigned long long>((size_t)p->B * p->N * soft_k);
    if (with_temp) b.tparts = ar.take<double>((size_t)p->max_iter * p->B * acc_blocks(p->N));
    b.bytes = mmk::align_up(ar.off, 256);
    return b;
}

// `code` is the entry's own: MMK_ERR_WORKSPACE, or MMK_ERR_ARG for mmk_icp_backward_points and mmk_icp_backward_hp.
int check_workspace(const char *who, int code, const void *ws, size_t have, size_t need)
{
    if (ws != nullptr && need <= have) return MMK_OK;
    mmk::set_error(code == MMK_ERR_ARG ? "%s: workspace too small (%zu < %zu bytes)" : "%s: workspace too small (%zu < %zu)", who, have,
                   need);
    return code;
}

// One dICP call as its entry received it, filled by position: an entry leaves out the tail it does not have.  The forward
// writes the histories, the backward only reads them.
struct IcpCall {
    const float *source, *target, *weight;
    int32_t *idx_hist;                     // (K | 1,B,N)
    float *T_hist;                         // (K+1,B,16)
    double *delta_hist, *A_hist;           // (K,B,6), (K,B,36)
    int32_t *active_hist;                  // (K+1,B)
    hipStream_t st;
    const float *hyper = nullptr;          // (1 | B, 3): k, trim_dist, trim_steep; NULL: the scalars of mmk_icp_params
    int hstride = 0;                       // 0 shared | 3 per pair
    const float *grad_T = nullptr;
    float *grad_weight = nullptr, *grad_T_init = nullptr;
    float *grad_source = nullptr, *grad_target = nullptr;      // (B,N,3), (B,M,tgt_cols)
    float *grad_hyper = nullptr;           // (B,3)
    int soft_k = 0;                        // > 0: soft correspondences (I2', I3''', I7'''); idx_hist is then (K | 1,B,N,k)
    float soft_temp = 0.f;
    const float *temp = nullptr;           // (1 | B): the device tau of the _soft_t entries; NULL: soft_temp
    int tstride = 0;                       // 0 shared | 1 per pair
    float *grad_temp = nullptr;            // (B)
};

// mmk_icp_soft as the _soft entries accept it: k in 2..8 with M >= k, temp finite and > 0.
int check_soft(const char *who, const mmk_icp_soft *s, int M)
{
    MMK_REQUIRE(s != nullptr, "%s: soft is NULL", who);
    MMK_REQUIRE(s->k >= 2 && s->k <= SOFT_KMAX, "%s: soft.k must be in 2..%d (got %d)", who, SOFT_KMAX, s->k);
    MMK_REQUIRE(M >= s->k, "%s: the target must have at least soft.k = %d rows (got M = %d)", who, s->k, M);
    MMK_REQUIRE(std::isfinite(s->temp) && s->temp > 0.f, "%s: soft.temp must be finite and > 0 (got %g)", who, (double)s->temp);
    return MMK_OK;
}

template <class T>
T *writable(const T *p) { return const_cast<T *>(p); }

// Bin `points` (B,M,cols) into the uniform grid of the exact searches (grid_nn_kernel, knn_normals_kernel).
int build_grid(const float *points, int B, int M, int cols, int dim, int32_t *counts, int32_t *cursor, int32_t *starts,
               float4 *sorted, hipStream_t st)
{
    MMK_CHECK_HIP(hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)B * GRID_NC * 2, st));   // counts and cursor
    hipLaunchKernelGGL(grid_count_kernel, dim3((M + 255) / 256, B), dim3(256), 0, st, points, M, cols, counts);
    MMK_LAUNCH_CHECK();
    hipLaunchKernelGGL(grid_scan_kernel, dim3(B), dim3(256), 0, st, counts, starts);
    MMK_LAUNCH_CHECK();
    hipLaunchKernelGGL(grid_fill_kernel, dim3((M + 255) / 256, B), dim3(256), 0, st, points, M, cols, dim, starts, cursor, sorted);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

template <int DIM, int TYPE>
int run_forward(const mmk_icp_params *p, const IcpCall &c, const IcpWs &w, int *iters_run, unsigned long long *soft_keys = nullptr)
{
    const int B = p->B, N = p->N, M = p->M;
    const float *const src = c.source, *const tgt = c.target;
    const hipStream_t st = c.st;
    const NNPlan pl = nn_plan(B, N, M, DIM);
    const int nblk = acc_blocks(N);
    const bool soft = c.soft_k > 0;
    SoftArgs sa{soft_keys, c.soft_k, c.soft_temp, c.temp, c.temp ? c.tstride : 0};
    // without saved state every iteration reuses one (B,N) buffer ((B,N,k) with soft correspondences)
    const size_t idx_step = p->save_state ? (size_t)B * N * (soft ? c.soft_k : 1) : 0;
    int k_done = 0;
    // (keys, status word, zero-row representatives: icp_init_kernel in mmk_icp_forward)
    const bool use_grid = p->nn_method == MMK_NN_GRID;
    const int nn_pts = NN_THREADS * pl.P;
    const bool dedup = !use_grid && pl.nsb <= 0xfff && B < (1 << 19);
    if (dedup) {
        hipLaunchKernelGGL(src_zero_scan_kernel, dim3(pl.nsb, B), dim3(NN_THREADS), 0, st, src, N, nn_pts, pl.nsb, w.allzero, w.zrep);
        MMK_LAUNCH_CHECK();
        hipLaunchKernelGGL(src_units_kernel, dim3(1), dim3(64), 0, st, w.allzero, w.zrep, B, pl.nsb, nn_pts, pl.ucap, w.ulist, w.ucnt);
        MMK_LAUNCH_CHECK();
    }
    const int32_t *az = dedup ? w.allzero : nullptr, *zr = dedup ? w.zrep : nullptr;
    if (use_grid) {   // the target is fixed over the iterations: bin it once
        const int rc = build_grid(tgt, B, M, p->tgt_cols, DIM, w.g_counts, w.g_cursor, w.g_starts, w.g_sorted, st);
        if (rc != MMK_OK) return rc;
    }
    const RobustArgs r = robust_args(p);
    const float *const hyper = c.hyper;
    const int hstride = hyper ? c.hstride : 0;     // without `hyper` (HP = false) the launch gets NULL, stride 0 and no check
    for (int it = 0; it < p->max_iter; ++it) {
        const float *Tk = c.T_hist + (size_t)it * B * 16;
        const int32_t *act = c.active_hist + (size_t)it * B;
        int32_t *idx = c.idx_hist + it * idx_step;
        // the correspondences of the previous iteration (still in the index buffer) bound the search / start the filter's bound
        const int32_t *prev = (it > 0) ? c.idx_hist + (it - 1) * idx_step : nullptr;
        unsigned long long *keys = w.packed + (size_t)(it & 1) * B * N, *keys_next = w.packed + (size_t)((it + 1) & 1) * B * N;
        if (use_grid) {
            const bool rec = g_prof.on && g_prof.n < g_prof.cap;
            if (rec) MMK_CHECK_HIP(hipEventRecord(g_prof.ev[2 * g_prof.n], st));
            if (soft)
                hipLaunchKernelGGL(grid_knn_kernel<DIM>, dim3((N + KNN_THREADS - 1) / KNN_THREADS, B), dim3(KNN_THREADS), 0, st, src, Tk,
                                   act, w.g_starts, w.g_sorted, N, M, c.soft_k, soft_keys);
            else
                hipLaunchKernelGGL(grid_nn_kernel<DIM>, dim3((N + 255) / 256, B), dim3(256), 0, st, src, Tk, act, w.g_starts,
                                   w.g_sorted, N, M, tgt, p->tgt_cols, prev, keys);
            MMK_LAUNCH_CHECK();
            if (rec) {
                MMK_CHECK_HIP(hipEventRecord(g_prof.ev[2 * g_prof.n + 1], st));
                g_prof.n++;
            }
        } else {
            int rc = launch_nn(DIM, src, w.tgtp, Tk, act, prev, dedup ? w.ulist : nullptr, w.ucnt, B, N, pl, keys, w.seed0, az, zr, w.tdec, st);
            if (rc != MMK_OK) return rc;
        }
        const int hcheck = hyper && it == 0 ? 1 : 0;
        sa.tcheck = c.temp && it == 0 ? 1 : 0;
        with_bools(hyper != nullptr, soft, [&](auto HP, auto SOFT) {
            if constexpr (!(HP() && SOFT()))        // (no entry combines the two)
                hipLaunchKernelGGL((icp_accumulate_kernel<DIM, TYPE, HP(), SOFT()>), dim3(nblk, B), dim3(ACC_THREADS), 0, st, src, tgt,
                                   p->tgt_cols, c.weight, Tk, act, keys, keys_next, az, zr, nn_pts, pl.nsb, idx, N, M, r.loss, r.k, r.k2,
                                   r.trim2, r.trim_dist, r.trim_steep, w.partials, w.status, hyper, hstride, hcheck, sa);
        });
        MMK_LAUNCH_CHECK();
        hipLaunchKernelGGL(icp_solve_kernel<DIM>, dim3(B), dim3(64), 0, st, w.partials, nblk, Tk,
                           c.T_hist + (size_t)(it + 1) * B * 16, c.delta_hist + (size_t)it * B * 6,
                           c.A_hist + (size_t)it * B * 36, act, c.active_hist + (size_t)(it + 1) * B, p->tolerance);
        MMK_LAUNCH_CHECK();
        k_done = it + 1;
        if (p->check_every > 0 && (k_done % p->check_every) == 0 && k_done < p->max_iter) {
            static thread_local int32_t host_act[1 << 16];
            MMK_REQUIRE(B <= (1 << 16), "mmk_icp_forward: check_every needs B <= 65536");
            MMK_CHECK_HIP(hipMemcpyAsync(host_act, c.active_hist + (size_t)k_done * B, sizeof(int32_t) * B,
                                         hipMemcpyDeviceToHost, st));
            MMK_CHECK_HIP(hipStreamSynchronize(st));
            bool any = false;
            for (int b = 0; b < B; ++b) any = any || host_act[b] != 0;
            if (!any) break;
        }
    }
    // iterations that were skipped after an early stop: carry the pose forward
    for (int it = k_done; it < p->max_iter; ++it) {
        MMK_CHECK_HIP(hipMemcpyAsync(c.T_hist + (size_t)(it + 1) * B * 16, c.T_hist + (size_t)it * B * 16,
                                     sizeof(float) * B * 16, hipMemcpyDeviceToDevice, st));
        MMK_CHECK_HIP(hipMemsetAsync(c.active_hist + (size_t)(it + 1) * B, 0, sizeof(int32_t) * B, st));
        MMK_CHECK_HIP(hipMemsetAsync(c.delta_hist + (size_t)it * B * 6, 0, sizeof(double) * B * 6, st));
    }
    if (iters_run) *iters_run = k_done;
    return MMK_OK;
}

template <int DIM, int TYPE>
int run_backward(const mmk_icp_params *p, const IcpCall &c, const IcpBwdWs &bw)
{
    const int B = p->B, N = p->N, M = p->M;
    const IcpWs &w = bw.w;
    const hipStream_t st = c.st;
    const int nblk = acc_blocks(N);
    const RobustArgs r = robust_args(p);
    constexpr int C = tgt_row_cols(DIM, TYPE), L = tgt_acc_cols(C);
    float *const gw = c.grad_weight, *const gsrc = c.grad_source, *const gtgt = c.grad_target;
    MMK_CHECK_HIP(hipMemsetAsync(gw, 0, sizeof(float) * (size_t)B * N, st));
    if (gsrc) MMK_CHECK_HIP(hipMemsetAsync(gsrc, 0, sizeof(float) * (size_t)B * N * 3, st));
    if (gtgt) {
        MMK_CHECK_HIP(hipMemsetAsync(bw.acc, 0, sizeof(unsigned long long) * (size_t)B * M * L, st));
        MMK_CHECK_HIP(hipMemsetAsync(bw.pmax, 0, sizeof(unsigned) * (size_t)B, st));
    }
    hipLaunchKernelGGL(f32_to_f64_kernel, dim3((B * 16 + 255) / 256), dim3(256), 0, st, c.grad_T, w.G0, B * 16);
    MMK_LAUNCH_CHECK();
    double *Gin = w.G0, *Gout = w.G1;
    int nparts = 0;
    // PTS: a cloud gradient is asked for; HP: the workspace has the hyper part, i.e. the entry was given `hyper`.  Without
    // PTS gsrc, rows and bw.pmax are all NULL, without HP c.hyper and hparts are: one argument list serves the four kernels.
    const bool pts = gsrc || gtgt, hp = bw.hparts != nullptr;
    const bool soft = c.soft_k > 0;                 // (never with hp: mmk_icp_backward_soft has no `hyper`)
    const int rpp = soft ? c.soft_k : 1;            // target rows (and saved indices) per point
    SoftArgs sa{nullptr, c.soft_k, c.soft_temp, c.temp, c.temp ? c.tstride : 0};
    for (int it = p->max_iter - 1; it >= 0; --it) {
        const float *Tk = c.T_hist + (size_t)it * B * 16;
        const int32_t *act = c.active_hist + (size_t)it * B;
        const double *delta = c.delta_hist + (size_t)it * B * 6;
        hipLaunchKernelGGL(icp_bwd_pair_kernel<DIM>, dim3(B), dim3(64), 0, st, Gin, w.partials, nparts, Tk, delta,
                           c.A_hist + (size_t)it * B * 36, act, Gout, w.lam);
        MMK_LAUNCH_CHECK();
        float *rows = gtgt ? bw.rows + (size_t)it * B * N * rpp * C : nullptr;
        double *hparts = hp ? bw.hparts + (size_t)it * B * nblk * 3 : nullptr;
        const int32_t *idx = c.idx_hist + (size_t)it * B * N * rpp;
        sa.tparts = bw.tparts ? bw.tparts + (size_t)it * B * nblk : nullptr;
        with_bools(pts, hp, [&](auto PTS, auto HP) {
            with_bool(soft, [&](auto SOFT) {
                if constexpr (!(HP() && SOFT()))    // (no entry combines the two)
                    hipLaunchKernelGGL((icp_bwd_point_kernel<DIM, TYPE, PTS(), HP(), SOFT()>), dim3(nblk, B), dim3(ACC_THREADS), 0, st,
                                       c.source, c.target, p->tgt_cols, c.weight, Tk, act, idx, w.lam, delta, N, M, r.loss, r.k, r.k2,
                                       r.trim2, r.trim_dist, r.trim_steep, gw, w.partials, gsrc, rows, bw.pmax, c.hyper, c.hstride,
                                       hparts, sa);
            });
        });
        MMK_LAUNCH_CHECK();
        nparts = nblk;
        std::swap(Gin, Gout);
    }
    if (c.grad_T_init) {
        hipLaunchKernelGGL(bwd_final_kernel<DIM>, dim3(B), dim3(64), 0, st, Gin, w.partials, nparts, c.grad_T_init);
        MMK_LAUNCH_CHECK();
    }
    if (c.grad_hyper) {
        hipLaunchKernelGGL(icp_bwd_hyper_final_kernel<3>, dim3(B), dim3(64), 0, st, bw.hparts, p->max_iter, B, nblk, c.grad_hyper);
        MMK_LAUNCH_CHECK();
    }
    if (c.grad_temp) {
        hipLaunchKernelGGL(icp_bwd_hyper_final_kernel<1>, dim3(B), dim3(64), 0, st, bw.tparts, p->max_iter, B, nblk, c.grad_temp);
        MMK_LAUNCH_CHECK();
    }
    if (gtgt) {
        int cnt_bits = 0;
        const int NR = N * rpp;                    // rows per pair and iteration: the scatter is flat over them
        while (((uint64_t)1 << cnt_bits) < (uint64_t)p->max_iter * (uint64_t)NR) ++cnt_bits;
        const unsigned gx = (unsigned)(((size_t)NR * L + ACC_THREADS - 1) / ACC_THREADS);
        hipLaunchKernelGGL(icp_bwd_target_scatter_kernel<C>, dim3(gx, B, p->max_iter), dim3(ACC_THREADS), 0, st, bw.rows, c.idx_hist,
                           c.active_hist, bw.pmax, B, NR, M, cnt_bits, bw.acc);
        MMK_LAUNCH_CHECK();
        hipLaunchKernelGGL(icp_bwd_target_final_kernel, dim3((M + 255) / 256, B), dim3(256), 0, st, bw.acc, bw.pmax, cnt_bits, M, DIM, C,
                           L, p->tgt_cols, gtgt);
        MMK_LAUNCH_CHECK();
    }
    return MMK_OK;
}

}  // namespace

// ================================================================================== C ABI
extern "C" int32_t mmk_nn_padded_m(int32_t M) { return (int32_t)mmk::align_up((size_t)std::max(M, 1), NN_TILE); }

extern "C" int mmk_pack_target(const float *target, int32_t B, int32_t M, int32_t tgt_cols, int32_t dim,
                               float *target_planar, void *stream)
{
    MMK_REQUIRE(target && target_planar, "mmk_pack_target: NULL pointer");
    MMK_REQUIRE(B >= 1 && M >= 1, "mmk_pack_target: B, M must be >= 1");
    MMK_REQUIRE((dim == 2 || dim == 3) && tgt_cols >= dim, "mmk_pack_target: dim must be 2|3 and <= tgt_cols");
    const int Mpad = mmk_nn_padded_m(M);
    hipLaunchKernelGGL(pack_target_kernel, dim3(Mpad / 256, B), dim3(256), 0, (hipStream_t)stream, target, M, tgt_cols,
                       dim, Mpad, target_planar, static_cast<float *>(nullptr), 1);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

extern "C" size_t mmk_nn_workspace_bytes(int32_t B, int32_t N, int32_t M, int32_t dim)
{
    (void)dim;
    if (B < 1 || N < 1 || M < 1) return 0;
    return mmk::align_up((size_t)B * N * sizeof(unsigned long long), 256) + mmk::align_up((size_t)B * N * sizeof(int32_t), 256) + 512;
}

extern "C" int mmk_nn_search(const float *source, const float *target_planar, const float *T, int32_t B, int32_t N,
                             int32_t M, int32_t dim, int32_t *idx, float *d2, void *workspace, size_t workspace_bytes,
                             void *stream)
{
    MMK_REQUIRE(source && target_planar && T && idx && d2, "mmk_nn_search: NULL pointer");
    MMK_REQUIRE(B >= 1 && N >= 1 && M >= 1, "mmk_nn_search: B, N, M must be >= 1");
    MMK_REQUIRE(dim == 2 || dim == 3, "mmk_nn_search: dim must be 2 or 3");
    const NNPlan pl = nn_plan(B, N, M, dim);
    mmk::Arena ar(workspace, workspace_bytes);
    unsigned long long *packed = ar.take<unsigned long long>((size_t)B * N);
    int32_t *seed0 = ar.take<int32_t>((size_t)B * N);
    if (!ar.ok() || workspace == nullptr) {
        mmk::set_error("mmk_nn_search: workspace too small (%zu < %zu)", workspace_bytes, ar.off);
        return MMK_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    MMK_CHECK_HIP(hipMemsetAsync(packed, 0xFF, sizeof(unsigned long long) * (size_t)B * N, st));
    int rc = launch_nn(dim, source, target_planar, T, nullptr, nullptr, nullptr, nullptr, B, N, pl, packed, seed0, nullptr, nullptr, nullptr, st);
    if (rc != MMK_OK) return rc;
    hipLaunchKernelGGL(nn_unpack_kernel, dim3((B * N + 255) / 256), dim3(256), 0, st, packed, B * N, idx, d2);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

namespace {

struct KnnWs {
    int32_t *counts, *cursor, *starts;
    float4 *sorted;
    size_t bytes;
};

KnnWs knn_carve(int32_t B, int32_t M, void *workspace, size_t workspace_bytes)
{
    mmk::Arena ar(workspace, workspace_bytes);
    KnnWs w;
    w.counts = ar.take<int32_t>((size_t)B * GRID_NC * 2);
    w.cursor = w.counts + (size_t)B * GRID_NC;
    w.starts = ar.take<int32_t>((size_t)B * (GRID_NC + 1));
    w.sorted = ar.take<float4>((size_t)B * M);
    w.bytes = mmk::align_up(ar.off, 256);
    return w;
}

template <int DIM, int KC>
void knn_launch(const float *points, int B, int M, int cols, int k, float max_radius, float pad_val, const float *viewpoint,
                const KnnWs &w, float *normals, float *curvature, int32_t *count, int32_t *nbr_idx, hipStream_t st)
{
    hipLaunchKernelGGL((knn_normals_kernel<DIM, KC>), dim3((M + KNN_THREADS - 1) / KNN_THREADS, B), dim3(KNN_THREADS), 0, st, points,
                       M, cols, k, max_radius, pad_val, viewpoint, w.starts, w.sorted, normals, curvature, count, nbr_idx);
}

}  // namespace

extern "C" size_t mmk_knn_normals_workspace_bytes(int32_t B, int32_t M)
{
    if (B < 1 || M < 1) return 0;
    return knn_carve(B, M, nullptr, 0).bytes;
}

extern "C" int mmk_knn_normals(const float *points, int32_t B, int32_t M, int32_t cols, int32_t dim, int32_t k, float max_radius,
                               float pad_val, const float *viewpoint, float *normals, float *curvature, int32_t *count,
                               int32_t *nbr_idx, void *workspace, size_t workspace_bytes, void *stream)
{
    MMK_REQUIRE(points && normals, "mmk_knn_normals: NULL pointer");
    MMK_REQUIRE(B >= 1 && M >= 1 && B <= 65535, "mmk_knn_normals: B must be in 1..65535 and M >= 1 (got %d, %d)", B, M);
    MMK_REQUIRE((dim == 2 || dim == 3) && cols >= dim, "mmk_knn_normals: dim must be 2|3 and <= cols");
    MMK_REQUIRE(k >= 3 && k <= 32, "mmk_knn_normals: k must be in 3..32 (got %d)", k);
    const KnnWs w = knn_carve(B, M, workspace, workspace_bytes);
    int rc = check_workspace("mmk_knn_normals", MMK_ERR_WORKSPACE, workspace, workspace_bytes, w.bytes);
    if (rc != MMK_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    // the grid of the ICP's exact search
    rc = build_grid(points, B, M, cols, dim, w.counts, w.cursor, w.starts, w.sorted, st);
    if (rc != MMK_OK) return rc;
#define KNN_GO(KC) knn_launch<D(), KC>(points, B, M, cols, k, max_radius, pad_val, viewpoint, w, normals, curvature, count, nbr_idx, st)
    with_dim(dim, [&](auto D) {
        if (k <= 8) KNN_GO(8);
        else if (k <= 16) KNN_GO(16);
        else KNN_GO(32);
    });
#undef KNN_GO
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

extern "C" int mmk_nn_profile_begin(int32_t capacity)
{
    MMK_REQUIRE(capacity >= 1 && capacity <= (1 << 20), "mmk_nn_profile_begin: bad capacity %d", capacity);
    if (g_prof.cap < capacity) {
        for (int i = 0; i < 2 * g_prof.cap; ++i) (void)hipEventDestroy(g_prof.ev[i]);
        delete[] g_prof.ev;
        g_prof.ev = new hipEvent_t[2 * (size_t)capacity];
        g_prof.cap = 0;
        for (int i = 0; i < 2 * capacity; ++i) MMK_CHECK_HIP(hipEventCreate(&g_prof.ev[i]));
        g_prof.cap = capacity;
    }
    g_prof.n = 0;
    g_prof.on = true;
    return MMK_OK;
}

extern "C" int mmk_nn_profile_end(float *ms_out, int32_t max_out, int32_t *n_out)
{
    MMK_REQUIRE(n_out != nullptr, "mmk_nn_profile_end: NULL n_out");
    g_prof.on = false;
    int n = g_prof.n;
    if (n > max_out) n = max_out;
    for (int i = 0; i < n; ++i) {
        MMK_CHECK_HIP(hipEventSynchronize(g_prof.ev[2 * i + 1]));
        MMK_CHECK_HIP(hipEventElapsedTime(&ms_out[i], g_prof.ev[2 * i], g_prof.ev[2 * i + 1]));
    }
    *n_out = g_prof.n;
    g_prof.n = 0;
    return MMK_OK;
}

extern "C" size_t mmk_icp_workspace_bytes(const mmk_icp_params *p)
{
    if (check_params(p) != MMK_OK) return 0;
    return carve_backward(p, false, false, nullptr, 0).bytes;    // = carve's: the forward and mmk_icp_backward share it
}

namespace {
// The params a call runs with: soft correspondences always search through the grid, whatever nn_method says.
mmk_icp_params effective_params(const mmk_icp_params *p, int soft_k)
{
    mmk_icp_params e = *p;
    if (soft_k > 0) e.nn_method = MMK_NN_GRID;
    return e;
}

// mmk_icp_forward (hyper NULL), mmk_icp_forward_hp and mmk_icp_forward_soft (c.soft_k > 0, already checked)
int forward_impl(const char *who, const mmk_icp_params *p_in, const IcpCall &c, const float *T_init, float *T_out, void *workspace,
                 size_t workspace_bytes, int *iters_run)
{
    int rc = check_params(p_in);
    if (rc != MMK_OK) return rc;
    MMK_REQUIRE(c.source && c.target && T_init && T_out && c.idx_hist && c.T_hist && c.delta_hist && c.A_hist && c.active_hist,
                "%s: NULL pointer", who);
    const mmk_icp_params eff = effective_params(p_in, c.soft_k), *const p = &eff;
    const IcpBwdWs fw = carve_backward(p, false, false, workspace, workspace_bytes, c.soft_k);     // the forward's part (+ the soft part)
    const IcpWs &w = fw.w;
    rc = check_workspace(who, MMK_ERR_WORKSPACE, workspace, workspace_bytes, fw.bytes);
    if (rc != MMK_OK) return rc;
    const hipStream_t st = c.st;
    const int B = p->B;
    {
        const int Mpad = mmk_nn_padded_m(p->M);
        hipLaunchKernelGGL(pack_target_kernel, dim3(Mpad / 256, B), dim3(256), 0, st, c.target, p->M, p->tgt_cols, p->dim, Mpad, w.tgtp,
                           w.tdec, NN_COARSE_STRIDE);
        MMK_LAUNCH_CHECK();
    }
    {
        const size_t nkeys = (size_t)2 * B * p->N;
        const unsigned blocks = (unsigned)std::min<size_t>(std::max<size_t>((nkeys + 255) / 256, (size_t)(B * 16 + 255) / 256), 2048);
        hipLaunchKernelGGL(icp_init_kernel, dim3(blocks), dim3(256), 0, st, w.packed, nkeys, w.status, c.active_hist, T_init, c.T_hist,
                           w.zrep, B, p->N);
        MMK_LAUNCH_CHECK();
    }
    rc = with_dim_type(p->dim, p->icp_type, [&](auto D, auto TYPE) { return run_forward<D(), TYPE()>(p, c, w, iters_run, fw.soft_keys); });
    if (rc != MMK_OK) return rc;
    MMK_CHECK_HIP(hipMemcpyAsync(T_out, c.T_hist + (size_t)p->max_iter * B * 16, sizeof(float) * B * 16,
                                 hipMemcpyDeviceToDevice, st));
    return MMK_OK;
}
}  // namespace

extern "C" int mmk_icp_forward(const mmk_icp_params *p, const float *source, const float *target,
                               const float *weight, const float *T_init, float *T_out, int32_t *idx_hist,
                               float *T_hist, double *delta_hist, double *A_hist, int32_t *active_hist,
                               void *workspace, size_t workspace_bytes, int *iters_run, void *stream)
{
    const IcpCall c{source, target, weight, idx_hist, T_hist, delta_hist, A_hist, active_hist, (hipStream_t)stream};
    return forward_impl("mmk_icp_forward", p, c, T_init, T_out, workspace, workspace_bytes, iters_run);
}

extern "C" int mmk_icp_forward_hp(const mmk_icp_params *p, const float *source, const float *target,
                                  const float *weight, const float *T_init, float *T_out, int32_t *idx_hist,
                                  float *T_hist, double *delta_hist, double *A_hist, int32_t *active_hist,
                                  const float *hyper, int32_t per_pair, void *workspace, size_t workspace_bytes,
                                  int *iters_run, void *stream)
{
    MMK_REQUIRE(per_pair == 0 || per_pair == 1, "mmk_icp_forward_hp: per_pair must be 0 or 1 (got %d)", per_pair);
    const IcpCall c{source, target, weight, idx_hist, T_hist, delta_hist, A_hist, active_hist, (hipStream_t)stream, hyper, per_pair ? 3 : 0};
    return forward_impl("mmk_icp_forward_hp", p, c, T_init, T_out, workspace, workspace_bytes, iters_run);
}

extern "C" size_t mmk_icp_soft_workspace_bytes(const mmk_icp_params *p, const mmk_icp_soft *soft)
{
    if (check_params(p) != MMK_OK || check_soft("mmk_icp_soft_workspace_bytes", soft, p->M) != MMK_OK) return 0;
    const mmk_icp_params eff = effective_params(p, soft->k);
    return carve_backward(&eff, false, false, nullptr, 0, soft->k).bytes;
}

extern "C" int mmk_icp_forward_soft(const mmk_icp_params *p, const float *source, const float *target,
                                    const float *weight, const float *T_init, float *T_out, int32_t *idx_hist,
                                    float *T_hist, double *delta_hist, double *A_hist, int32_t *active_hist,
                                    const mmk_icp_soft *soft, void *workspace, size_t workspace_bytes, int *iters_run,
                                    void *stream)
{
    int rc = check_params(p);
    if (rc != MMK_OK) return rc;
    rc = check_soft("mmk_icp_forward_soft", soft, p->M);
    if (rc != MMK_OK) return rc;
    IcpCall c{source, target, weight, idx_hist, T_hist, delta_hist, A_hist, active_hist, (hipStream_t)stream};
    c.soft_k = soft->k;
    c.soft_temp = soft->temp;
    return forward_impl("mmk_icp_forward_soft", p, c, T_init, T_out, workspace, workspace_bytes, iters_run);
}

// mmk_icp_forward_soft with tau on the device (I3⁗): `temp` (1 | B), per_pair 0 | 1.  temp NULL: mmk_icp_forward_soft.
extern "C" int mmk_icp_forward_soft_t(const mmk_icp_params *p, const float *source, const float *target,
                                      const float *weight, const float *T_init, float *T_out, int32_t *idx_hist,
                                      float *T_hist, double *delta_hist, double *A_hist, int32_t *active_hist,
                                      const mmk_icp_soft *soft, const float *temp, int32_t per_pair, void *workspace,
                                      size_t workspace_bytes, int *iters_run, void *stream)
{
    int rc = check_params(p);
    if (rc != MMK_OK) return rc;
    rc = check_soft("mmk_icp_forward_soft_t", soft, p->M);
    if (rc != MMK_OK) return rc;
    MMK_REQUIRE(per_pair == 0 || per_pair == 1, "mmk_icp_forward_soft_t: per_pair must be 0 or 1 (got %d)", per_pair);
    IcpCall c{source, target, weight, idx_hist, T_hist, delta_hist, A_hist, active_hist, (hipStream_t)stream};
    c.soft_k = soft->k;
    c.soft_temp = soft->temp;
    c.temp = temp;
    c.tstride = per_pair ? 1 : 0;
    return forward_impl("mmk_icp_forward_soft_t", p, c, T_init, T_out, workspace, workspace_bytes, iters_run);
}

extern "C" int mmk_icp_status(const mmk_icp_params *p, const void *workspace, size_t workspace_bytes, int32_t *status_out,
                              void *stream)
{
    int rc = check_params(p);
    if (rc != MMK_OK) return rc;
    MMK_REQUIRE(status_out != nullptr, "mmk_icp_status: NULL status_out");
    const IcpWs w = carve(p, const_cast<void *>(workspace), workspace_bytes);
    rc = check_workspace("mmk_icp_status", MMK_ERR_WORKSPACE, workspace, workspace_bytes, w.bytes);
    if (rc != MMK_OK) return rc;
    MMK_CHECK_HIP(hipMemcpyAsync(status_out, w.status, sizeof(int32_t), hipMemcpyDefault, (hipStream_t)stream));
    return MMK_OK;
}

extern "C" size_t mmk_icp_partials_count(const mmk_icp_params *p)
{
    if (check_params(p) != MMK_OK) return 0;
    return (size_t)p->B * acc_blocks(p->N) * nacc(p->dim);
}

extern "C" int mmk_icp_accumulate(const mmk_icp_params *p, const float *source, const float *target, const float *weight,
                                  const float *T, const uint64_t *nn_keys, int32_t *idx_out, double *partials, int32_t *status,
                                  void *stream)
{
    int rc = check_params(p);
    if (rc != MMK_OK) return rc;
    MMK_REQUIRE(source && target && T && nn_keys && idx_out && partials && status, "mmk_icp_accumulate: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    const unsigned long long *keys = reinterpret_cast<const unsigned long long *>(nn_keys);
    const RobustArgs r = robust_args(p);
    // one step on its own: every pair active, no keys to arm for a next search, no zero-row bookkeeping, no hyper array
    const int32_t *const none = nullptr;
    unsigned long long *const no_next = nullptr;
    const float *const no_hyper = nullptr;
    with_dim_type(p->dim, p->icp_type, [&](auto D, auto TYPE) {
        hipLaunchKernelGGL((icp_accumulate_kernel<D(), TYPE(), false>), dim3(acc_blocks(p->N), p->B), dim3(ACC_THREADS), 0, st, source,
                           target, p->tgt_cols, weight, T, none, keys, no_next, none, none, 1, 1, idx_out, p->N, p->M, r.loss, r.k, r.k2,
                           r.trim2, r.trim_dist, r.trim_steep, partials, status, no_hyper, 0, 0, SoftArgs{nullptr, 0, 0.f});
    });
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

extern "C" int mmk_icp_solve_update(const mmk_icp_params *p, const double *partials, const float *T_in, float *T_out,
                                    double *delta_out, double *A_out, const int32_t *active_in, int32_t *active_out, void *stream)
{
    int rc = check_params(p);
    if (rc != MMK_OK) return rc;
    MMK_REQUIRE(partials && T_in && T_out && delta_out && A_out && active_in && active_out, "mmk_icp_solve_update: NULL pointer");
    with_dim(p->dim, [&](auto D) {
        hipLaunchKernelGGL(icp_solve_kernel<D()>, dim3(p->B), dim3(64), 0, (hipStream_t)stream, partials, acc_blocks(p->N), T_in, T_out,
                           delta_out, A_out, active_in, active_out, p->tolerance);
    });
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

namespace {
// The three backward entries.  `per_pair` is mmk_icp_backward_hp's argument (0 from the others); a gradient output an entry
// does not have is NULL in `c` and its check holds.  `ws_code`: what the entry returns for a short workspace.
int backward_impl(const char *who, int ws_code, const mmk_icp_params *p_in, const IcpCall &c, int per_pair, void *workspace,
                  size_t workspace_bytes)
{
    int rc = check_params(p_in);
    if (rc != MMK_OK) return rc;
    const mmk_icp_params eff = effective_params(p_in, c.soft_k), *const p = &eff;
    MMK_REQUIRE(p->save_state, "%s: forward must have run with save_state = 1", who);
    MMK_REQUIRE(c.source && c.target && c.idx_hist && c.T_hist && c.delta_hist && c.A_hist && c.active_hist && c.grad_T && c.grad_weight,
                "%s: NULL pointer", who);
    MMK_REQUIRE(per_pair == 0 || per_pair == 1, "%s: per_pair must be 0 or 1 (got %d)", who, per_pair);
    MMK_REQUIRE(c.grad_hyper == nullptr || c.hyper != nullptr, "%s: grad_hyper needs hyper", who);
    MMK_REQUIRE(c.grad_temp == nullptr || c.temp != nullptr, "%s: grad_temp needs temp", who);
    MMK_REQUIRE(c.grad_target == nullptr || p->max_iter <= 65535, "%s: the target gradient needs max_iter <= 65535 (got %d)", who,
                p->max_iter);
    const IcpBwdWs bw = carve_backward(p, c.grad_target != nullptr, c.hyper != nullptr, workspace, workspace_bytes, c.soft_k,
                                       c.grad_temp != nullptr);
    rc = check_workspace(who, ws_code, workspace, workspace_bytes, bw.bytes);
    if (rc != MMK_OK) return rc;
    return with_dim_type(p->dim, p->icp_type, [&](auto D, auto TYPE) { return run_backward<D(), TYPE()>(p, c, bw); });
}
}  // namespace

// No cloud and no hyper-parameter gradients; a short workspace is MMK_ERR_WORKSPACE.
extern "C" int mmk_icp_backward(const mmk_icp_params *p, const float *source, const float *target,
                                const float *weight, const int32_t *idx_hist, const float *T_hist,
                                const double *delta_hist, const double *A_hist, const int32_t *active_hist,
                                const float *grad_T, float *grad_weight, float *grad_T_init, void *workspace,
                                size_t workspace_bytes, void *stream)
{
    const IcpCall c{source, target, weight, writable(idx_hist), writable(T_hist), writable(delta_hist), writable(A_hist),
                    writable(active_hist), (hipStream_t)stream, nullptr, 0, grad_T, grad_weight, grad_T_init};
    return backward_impl("mmk_icp_backward", MMK_ERR_WORKSPACE, p, c, 0, workspace, workspace_bytes);
}

extern "C" size_t mmk_icp_backward_points_workspace_bytes(const mmk_icp_params *p, int32_t with_target)
{
    if (check_params(p) != MMK_OK) return 0;
    return carve_backward(p, with_target != 0, false, nullptr, 0).bytes;
}

// No hyper-parameter array or gradient; a short workspace is MMK_ERR_ARG.
extern "C" int mmk_icp_backward_points(const mmk_icp_params *p, const float *source, const float *target,
                                       const float *weight, const int32_t *idx_hist, const float *T_hist,
                                       const double *delta_hist, const double *A_hist, const int32_t *active_hist,
                                       const float *grad_T, float *grad_weight, float *grad_T_init, float *grad_source,
                                       float *grad_target, void *workspace, size_t workspace_bytes, void *stream)
{
    const IcpCall c{source, target, weight, writable(idx_hist), writable(T_hist), writable(delta_hist), writable(A_hist),
                    writable(active_hist), (hipStream_t)stream, nullptr, 0, grad_T, grad_weight, grad_T_init, grad_source, grad_target};
    return backward_impl("mmk_icp_backward_points", MMK_ERR_ARG, p, c, 0, workspace, workspace_bytes);
}

extern "C" size_t mmk_icp_backward_hp_workspace_bytes(const mmk_icp_params *p, int32_t with_target, int32_t with_hyper)
{
    if (check_params(p) != MMK_OK) return 0;
    return carve_backward(p, with_target != 0, with_hyper != 0, nullptr, 0).bytes;
}

// Every gradient the caller passes; hyper NULL: the scalars of p (grad_hyper then must be NULL).  A short workspace is
// MMK_ERR_ARG.
extern "C" int mmk_icp_backward_hp(const mmk_icp_params *p, const float *source, const float *target,
                                   const float *weight, const int32_t *idx_hist, const float *T_hist,
                                   const double *delta_hist, const double *A_hist, const int32_t *active_hist,
                                   const float *grad_T, float *grad_weight, float *grad_T_init, float *grad_source,
                                   float *grad_target, const float *hyper, int32_t per_pair, float *grad_hyper,
                                   void *workspace, size_t workspace_bytes, void *stream)
{
    const IcpCall c{source, target, weight, writable(idx_hist), writable(T_hist), writable(delta_hist), writable(A_hist),
                    writable(active_hist), (hipStream_t)stream, hyper, per_pair ? 3 : 0, grad_T, grad_weight, grad_T_init,
                    grad_source, grad_target, grad_hyper};
    return backward_impl("mmk_icp_backward_hp", MMK_ERR_ARG, p, c, per_pair, workspace, workspace_bytes);
}

extern "C" size_t mmk_icp_backward_soft_workspace_bytes(const mmk_icp_params *p, const mmk_icp_soft *soft, int32_t with_target)
{
    if (check_params(p) != MMK_OK || check_soft("mmk_icp_backward_soft_workspace_bytes", soft, p->M) != MMK_OK) return 0;
    const mmk_icp_params eff = effective_params(p, soft->k);
    return carve_backward(&eff, with_target != 0, false, nullptr, 0, soft->k).bytes;
}

// The reverse sweep of a mmk_icp_forward_soft call (I7'''): grad_source and grad_target each optional, idx_hist (K,B,N,k).
// A short workspace is MMK_ERR_ARG.
extern "C" int mmk_icp_backward_soft(const mmk_icp_params *p, const float *source, const float *target,
                                     const float *weight, const int32_t *idx_hist, const float *T_hist,
                                     const double *delta_hist, const double *A_hist, const int32_t *active_hist,
                                     const float *grad_T, float *grad_weight, float *grad_T_init, float *grad_source,
                                     float *grad_target, const mmk_icp_soft *soft, void *workspace, size_t workspace_bytes,
                                     void *stream)
{
    int rc = check_params(p);
    if (rc != MMK_OK) return rc;
    rc = check_soft("mmk_icp_backward_soft", soft, p->M);
    if (rc != MMK_OK) return rc;
    IcpCall c{source, target, weight, writable(idx_hist), writable(T_hist), writable(delta_hist), writable(A_hist),
              writable(active_hist), (hipStream_t)stream, nullptr, 0, grad_T, grad_weight, grad_T_init, grad_source, grad_target};
    c.soft_k = soft->k;
    c.soft_temp = soft->temp;
    return backward_impl("mmk_icp_backward_soft", MMK_ERR_ARG, p, c, 0, workspace, workspace_bytes);
}

extern "C" size_t mmk_icp_backward_soft_t_workspace_bytes(const mmk_icp_params *p, const mmk_icp_soft *soft, int32_t with_target,
                                                          int32_t with_temp)
{
    if (check_params(p) != MMK_OK || check_soft("mmk_icp_backward_soft_t_workspace_bytes", soft, p->M) != MMK_OK) return 0;
    const mmk_icp_params eff = effective_params(p, soft->k);
    return carve_backward(&eff, with_target != 0, false, nullptr, 0, soft->k, with_temp != 0).bytes;
}

// The reverse sweep of a mmk_icp_forward_soft_t call (I7⁗): mmk_icp_backward_soft plus the device tau and grad_temp (B, one
// row per pair also when tau is shared; optional).  temp NULL and grad_temp NULL: mmk_icp_backward_soft.  A short workspace
// is MMK_ERR_ARG.
extern "C" int mmk_icp_backward_soft_t(const mmk_icp_params *p, const float *source, const float *target,
                                       const float *weight, const int32_t *idx_hist, const float *T_hist,
                                       const double *delta_hist, const double *A_hist, const int32_t *active_hist,
                                       const float *grad_T, float *grad_weight, float *grad_T_init, float *grad_source,
                                       float *grad_target, const mmk_icp_soft *soft, const float *temp, int32_t per_pair,
                                       float *grad_temp, void *workspace, size_t workspace_bytes, void *stream)
{
    int rc = check_params(p);
    if (rc != MMK_OK) return rc;
    rc = check_soft("mmk_icp_backward_soft_t", soft, p->M);
    if (rc != MMK_OK) return rc;
    IcpCall c{source, target, weight, writable(idx_hist), writable(T_hist), writable(delta_hist), writable(A_hist),
              writable(active_hist), (hipStream_t)stream, nullptr, 0, grad_T, grad_weight, grad_T_init, grad_source, grad_target};
    c.soft_k = soft->k;
    c.soft_temp = soft->temp;
    c.temp = temp;
    c.tstride = per_pair ? 1 : 0;
    c.grad_temp = grad_temp;
    return backward_impl("mmk_icp_backward_soft_t", MMK_ERR_ARG, p, c, per_pair, workspace, workspace_bytes);
}

namespace {
struct KnnSearchWs {
    KnnWs grid;
    unsigned long long *keys;      // (B,N,k)
    size_t bytes;
};

KnnSearchWs knn_search_carve(int32_t B, int32_t N, int32_t M, int32_t k, void *workspace, size_t workspace_bytes)
{
    KnnSearchWs w;
    w.grid = knn_carve(B, M, workspace, workspace_bytes);
    mmk::Arena ar(workspace, workspace_bytes);
    ar.off = w.grid.bytes;
    w.keys = ar.take<unsigned long long>((size_t)B * N * k);
    w.bytes = mmk::align_up(ar.off, 256);
    return w;
}

int check_knn_search(const char *who, int32_t B, int32_t N, int32_t M, int32_t k)
{
    MMK_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && M >= 1, "%s: B must be in 1..65535, N and M >= 1 (got %d, %d, %d)", who, B, N, M);
    MMK_REQUIRE(k >= 2 && k <= SOFT_KMAX, "%s: k must be in 2..%d (got %d)", who, SOFT_KMAX, k);
    MMK_REQUIRE(M >= k, "%s: the target must have at least k = %d rows (got M = %d)", who, k, M);
    return MMK_OK;
}
}  // namespace

extern "C" size_t mmk_knn_search_workspace_bytes(int32_t B, int32_t N, int32_t M, int32_t k)
{
    if (check_knn_search("mmk_knn_search_workspace_bytes", B, N, M, k) != MMK_OK) return 0;
    return knn_search_carve(B, N, M, k, nullptr, 0).bytes;
}

// I2' on its own: the k nearest rows of `target` (B,M,tgt_cols) to the transformed source points, in key order.
extern "C" int mmk_knn_search(const float *source, const float *target, const float *T, int32_t B, int32_t N, int32_t M,
                              int32_t tgt_cols, int32_t dim, int32_t k, int32_t *idx, float *d2, void *workspace,
                              size_t workspace_bytes, void *stream)
{
    MMK_REQUIRE(source && target && T && idx && d2, "mmk_knn_search: NULL pointer");
    MMK_REQUIRE((dim == 2 || dim == 3) && tgt_cols >= dim, "mmk_knn_search: dim must be 2|3 and <= tgt_cols");
    int rc = check_knn_search("mmk_knn_search", B, N, M, k);
    if (rc != MMK_OK) return rc;
    MMK_REQUIRE((size_t)B * N * k <= 0x7fffffffu, "mmk_knn_search: B * N * k must fit 31 bits");
    const KnnSearchWs w = knn_search_carve(B, N, M, k, workspace, workspace_bytes);
    rc = check_workspace("mmk_knn_search", MMK_ERR_WORKSPACE, workspace, workspace_bytes, w.bytes);
    if (rc != MMK_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = build_grid(target, B, M, tgt_cols, dim, w.grid.counts, w.grid.cursor, w.grid.starts, w.grid.sorted, st);
    if (rc != MMK_OK) return rc;
    const int32_t *const every_pair = nullptr;
    with_dim(dim, [&](auto D) {
        hipLaunchKernelGGL(grid_knn_kernel<D()>, dim3((N + KNN_THREADS - 1) / KNN_THREADS, B), dim3(KNN_THREADS), 0, st, source, T,
                           every_pair, w.grid.starts, w.grid.sorted, N, M, k, w.keys);
    });
    MMK_LAUNCH_CHECK();
    const int n = B * N * k;
    hipLaunchKernelGGL(nn_unpack_kernel, dim3((n + 255) / 256), dim3(256), 0, st, w.keys, n, idx, d2);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}
