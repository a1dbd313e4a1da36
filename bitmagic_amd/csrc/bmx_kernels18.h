// bmx_kernels18.h -- a batch of range COUNTS over a resident bit-sliced column: the walk of k_slice_compare (bmx_kernels4.h)
// carried for T thresholds at once, so that every loaded plane word serves T bounds (bmx_slice_range_counts).
#pragma once
#include "bmx_kernels17.h"

// ---------------------------------------------------------------------------
// Reference: no batch call.  Its users loop sparse_vector_scanner::find_range / find_gt / find_le and take count()
// (src/bmsparsevec_algo.h:1135-1174, 2690-2900; signed containers: find_gt_horizontal_s :1484, 3033-3160) -- one chain of
// whole-vector passes per range.  bmx_slice_compare makes that one pass over the planes per range; a batch of n ranges over
// the same column still reads every plane n times.
// Here: the host turns the ranges into sorted distinct thresholds t and asks for LE(t) = valid rows whose magnitude is <= t;
// every count is a difference of two of them (bmx.hip, range_plan).  The walk is bit-serial and independent per bound:
//     bit b of t set   : eq_t &= P            clear : gt_t |= eq_t & P;  eq_t &= ~P          (planes from the top bit down)
// written without a branch as  x = eq_t & P;  gt_t |= x & m;  eq_t = (eq_t & m) ^ x  with the wave-uniform mask m = bit ? 0 : ~0
// (four VALU operations per word where the branch form averages two: with a branch per threshold the compiler kept the old and
// the new state of every accumulator across the loop edge -- 20 VGPRs per threshold instead of 8).
//     LE(t) = popcount(~gt_t & V),  V = rows [0, size) of the piece AND the not-NULL block;  SGN: split by the sign block S
// The walk is unrolled over t; a plane word is loaded once and used T times.
// State: a whole-block accumulator pair costs 64 VGPRs per bound (k_slice_compare<true>: 282 VGPRs for two), so a wave works
// on a Part<RP> piece of a block column -- RP = 1: 8 VGPRs per threshold -- and the (column, piece) items are dealt to a
// persistent grid; the walk of a piece stops when no row is equal-so-far for ANY threshold (one ballot per plane).
// Operands: the host expands every operand that holds GAP blocks to raw words first (k_vec_expand, as bmx_slice_eq_counts
// does): a GAP block decodes WHOLE (32 VGPRs + 8 KiB of LDS per wave), and with 1-KiB pieces that would be eight decodes per
// plane block next to the accumulators.  What reaches this kernel is bit-blocks, FULL and NULL blocks, or raw words.
// Counts: per-lane partial sums over all the items of a wave, one wave reduction and one LDS fold per workgroup at the end,
// then ONE 64-bit atomicAdd per threshold per workgroup.  Integer adds: the result does not depend on the order.
// ---------------------------------------------------------------------------
struct LeOperand { const u64* desc; const uint4* raw; u32 nblk; u32 pad; };   // raw != null: ncols expanded blocks; else the descriptor table
template <int T> struct LeThresholds { u64 t[T]; };

// piece h (RP KiB) of block column c of operand i -> its block kind (K_NULL: P = zeros; K_FULL: P = ones)
template <int RP>
__device__ __forceinline__ u32 le_piece(const LeOperand* __restrict__ ops, u32 i, u32 c, u32 h, Part<RP>& P, u32 lane)
{
    const uint4* raw = (const uint4*)uniform64((u64)(uintptr_t)ops[i].raw);
    if (raw) { part_load<RP, false>(P, as_gc4(raw + (size_t)c * 512u) + h * (u32)RP * 64u, lane); return K_BIT; }
    const u64* dt = (const u64*)uniform64((u64)(uintptr_t)ops[i].desc);
    const u64 d = (dt && c < uniform32(ops[i].nblk)) ? uniform64(dt[c]) : 0ull;
    const u32 k = DESC_K(d);
    if (k == K_BIT) { part_load<RP, false>(P, as_gc4(DESC_P(d)) + h * (u32)RP * 64u, lane); return K_BIT; }
#pragma unroll
    for (int r = 0; r < RP; ++r) P.r[r] = (u32x4)(k == K_FULL ? ~0u : 0u);
    return k == K_FULL ? K_FULL : K_NULL;                                                   // (a GAP block cannot come here: the host expanded its operand)
}

__device__ __forceinline__ u32 popc128(u32x4 v) { return (u32)__popcll(((u64)v.y << 32) | v.x) + (u32)__popcll(((u64)v.w << 32) | v.z); }

// ops[0 .. nplanes) = magnitude planes, ops[nplanes] = the sign plane (SGN), ops[nplanes + 1] = the not-NULL vector (has_nn).
// counts[j] (SGN: counts[2j] sign clear, counts[2j + 1] sign set) += LE(thr.t[j]) for j < nthr; totals[0] (SGN: [0], [1]) +=
// valid rows, when totals != null; *stat += the plane, sign and not-NULL bytes the launch loaded, when stat != null.  Every
// threshold is below 2^nplanes (the host resolves the others).
template <int T, int RP, bool SGN>
__global__ __launch_bounds__(256)
void k_slice_le_counts(const LeOperand* __restrict__ ops, u32 nplanes, u32 ncols, LeThresholds<T> thr, u32 nthr, u64 size, int has_nn,
                       u64* __restrict__ counts, u64* __restrict__ totals, u64* __restrict__ stat)
{
    constexpr u32 NPIECE = 8u / (u32)RP;
    constexpr int NC = SGN ? 2 : 1, NACC = NC * (T + 1);
    __shared__ u32 red[4][NACC];
    const u32 lane = lane_id(), wave = threadIdx.x >> 6;
    u32 acc[NACC];                                                     // [NC * j + s]; the last NC: valid rows
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0u;
    const u32 nitems = ncols * NPIECE;
    u32 read_bytes = 0;                                                // (wave-uniform: a scalar)
    u64 thr_or = 0ull;                                                 // a plane of zeros matters only under a SET bit of some threshold
#pragma unroll
    for (int j = 0; j < T; ++j) thr_or |= (u32)j < nthr ? thr.t[j] : 0ull;
    for (u32 w = uniform32(blockIdx.x * 4u + wave); w < nitems; w += gridDim.x * 4u) {
        const u32 c = w / NPIECE, h = w % NPIECE;
        const u64 base = (u64)c << 16;
        const u32 lim = size <= base ? 0u : (size - base >= 65536ull ? 65536u : (u32)(size - base));
        Part<RP> gt[T], eq[T];
#pragma unroll
        for (int j = 0; j < T; ++j) {
#pragma unroll
            for (int r = 0; r < RP; ++r) { gt[j].r[r] = (u32x4)(0u); eq[j].r[r] = (u32x4)((u32)j < nthr ? ~0u : 0u); }
        }
        bool live = nthr != 0u && lim != 0u;
        for (u32 b = nplanes; b-- > 0u && live; ) {
            Part<RP> P;
            const u32 k = le_piece<RP>(ops, b, c, h, P, lane);
            read_bytes += k == K_BIT ? (u32)RP * 1024u : 0u;
            if (k == K_NULL && !((thr_or >> b) & 1ull)) continue;       // P = 0 under a clear bit of every threshold: nothing changes
#pragma unroll
            for (int j = 0; j < T; ++j) {
                const u32 m = ((thr.t[j] >> b) & 1ull) ? 0u : ~0u;      // wave-uniform: a scalar select, the update itself has no branch
#pragma unroll
                for (int r = 0; r < RP; ++r) {
                    const u32x4 x = eq[j].r[r] & P.r[r];                // bit set: eq = x;   clear: gt |= x, eq ^= x
                    gt[j].r[r] |= x & m;
                    eq[j].r[r] = (eq[j].r[r] & m) ^ x;
                }
            }
            u32 any = 0u;
#pragma unroll
            for (int j = 0; j < T; ++j) {
#pragma unroll
                for (int r = 0; r < RP; ++r) { const u32x4 t = eq[j].r[r]; any |= t.x | t.y | t.z | t.w; }
            }
            live = __ballot(any != 0u) != 0ull;
        }
        // V = rows [0, size) of this piece, not NULL; S = the sign block
        Part<RP> V, S;
        if (has_nn) read_bytes += le_piece<RP>(ops, nplanes + 1u, c, h, V, lane) == K_BIT ? (u32)RP * 1024u : 0u;
        if constexpr (SGN) read_bytes += le_piece<RP>(ops, nplanes, c, h, S, lane) == K_BIT ? (u32)RP * 1024u : 0u;
#pragma unroll
        for (int r = 0; r < RP; ++r) {
            const u32 w0 = (((h * (u32)RP + (u32)r) * 256u + lane * 4u) << 5);    // first row of word .x
            u32 ws[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { const u32 lo = w0 + (u32)q * 32u; ws[q] = lim >= lo + 32u ? ~0u : (lim <= lo ? 0u : ((1u << (lim - lo)) - 1u)); }
            u32x4 m; m.x = ws[0]; m.y = ws[1]; m.z = ws[2]; m.w = ws[3];
            V.r[r] = has_nn ? (V.r[r] & m) : m;
        }
#pragma unroll
        for (int j = 0; j <= T; ++j) {                                 // j == T: the valid rows themselves
#pragma unroll
            for (int r = 0; r < RP; ++r) {
                u32x4 le = V.r[r];
                if (j < T) le &= ~gt[j < T ? j : 0].r[r];
                if constexpr (SGN) { acc[2 * j] += popc128(le & ~S.r[r]); acc[2 * j + 1] += popc128(le & S.r[r]); }
                else acc[j] += popc128(le);
            }
        }
    }
    if (stat && lane == 0 && read_bytes) atomicAdd(reinterpret_cast<unsigned long long*>(stat), (unsigned long long)read_bytes);
#pragma unroll
    for (int k = 0; k < NACC; ++k) {
        const u32 s = wave_sum(acc[k]);
        if (lane == 0) red[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < (u32)NACC) {
        const u32 k = threadIdx.x;
        const u64 s = (u64)red[0][k] + red[1][k] + red[2][k] + red[3][k];
        if (s) {
            if (k < (u32)(NC * T)) { if (k / (u32)NC < nthr) atomicAdd(reinterpret_cast<unsigned long long*>(counts + k), (unsigned long long)s); }
            else if (totals) atomicAdd(reinterpret_cast<unsigned long long*>(totals + (k - (u32)(NC * T))), (unsigned long long)s);
        }
    }
}
