// bmx_kernels17.h -- which rows differ between two resident bit-sliced columns: sparse_vector_find_mismatch /
// sparse_vector_find_first_mismatch (src/bmsparsevec_algo.h:656-792, 478-636) in one walk over both columns' planes.
#pragma once
#include "bmx_kernels16.h"

// ---------------------------------------------------------------------------
// Reference: per plane pair a whole-vector XOR into a temporary and an OR of the temporary into the result (:693-715),
// then set_range for the size difference (:716-731) and one to three more whole-vector passes for the NULL rule
// (:740-788) -- about 4P+1 block transfers per block column and P temporaries of the full length.
// Here: ONE pass.  A wave owns a block column, walks the plane pairs and keeps D = OR_i (A_i ^ B_i) as a register image;
// every plane block is read once (2P reads), nothing intermediate touches HBM, and the walk stops once D covers every row
// of the column (no further plane can add a row).  Then, on the same registers:
//     D |= ones[size_lo, size_hi)                                    the rows only the longer column has
//     NULL term   MM_NULL_NONE    nothing
//                 MM_NULL_AND_OR  D &= (N_a | N_b)                   an absent not-NULL vector counts as all zeros
//                 MM_NULL_OR_XOR  D |= (N_a ^ N_b)                   an absent one counts as ones[0, fill)
//     D &= ones[0, size_hi)
// and one of three endings: the block is stored (store_result's rule), counted, or its lowest set bit goes into *best.
// The first mismatch of the reference has no size-difference term: the host passes size_lo == size_hi for it.
// Operand table (operand_list / direct_table): rows [0, P) planes of a, [P, 2P) planes of b, 2P = N_a, 2P + 1 = N_b;
// a null row is a plane / vector that does not exist.
// ---------------------------------------------------------------------------
enum { MM_NULL_NONE = 0, MM_NULL_AND_OR = 1, MM_NULL_OR_XOR = 2 };
enum { MM_STORE = 0, MM_COUNT = 1, MM_FIRST = 2 };

// does D hold every row [0, lim) of its block?  (lim = 1..65536; wave-uniform answer)
__device__ __forceinline__ bool blk_covers_rows(const Blk& D, u32 lim, u32 lane)
{
    if (lim >= 65536u) return blk_is_ones(D);
    u32 miss = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        u32 w0 = ((u32)i * 256u + lane * 4u) << 5;                 // first row of word .x
        u32 w[4] = {D.r[i].x, D.r[i].y, D.r[i].z, D.r[i].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            u32 lo = w0 + (u32)j * 32u;
            u32 m = lim >= lo + 32u ? ~0u : (lim <= lo ? 0u : ((1u << (lim - lo)) - 1u));
            miss |= m & ~w[j];
        }
    }
    return __ballot(miss != 0u) == 0ull;
}

// descriptor of block nb of operand row i (0 = the row does not exist, or ends before nb)
__device__ __forceinline__ u64 mm_desc(const u64* const* __restrict__ descs, const u32* __restrict__ nblk, u32 i, u32 nb)
{
    const u64* dt = (const u64*)uniform64((u64)(uintptr_t)descs[i]);
    return (dt && nb < uniform32(nblk[i])) ? uniform64(dt[nb]) : 0ull;
}

__global__ __launch_bounds__(256)
void k_slice_mismatch(const u64* const* __restrict__ descs, const u32* __restrict__ nblk, u32 nplanes /* P */,
                      u32 col_from, u32 col_to, u64 size_lo, u64 size_hi, int null_mode, u64 fill, int ending, int xcd_swz,
                      uint4* __restrict__ slab, u64* __restrict__ desc, BlockStat* __restrict__ st, u64* __restrict__ slots,
                      u64* __restrict__ best)
{
    __shared__ u32 lds[4 * 2048];
    u32 lane = lane_id(), wave = threadIdx.x >> 6;
    u32 bid = (xcd_swz && ending != MM_FIRST) ? xcd_remap(blockIdx.x, gridDim.x) : blockIdx.x;
    u32 nb = uniform32(col_from + bid * 4u + wave);
    u32 cnt = 0;
    bool work = nb < col_to;
    // first mismatch: an earlier column already has a hit (*best only moves down)
    if (work && ending == MM_FIRST && ((u64)nb << 16) > __hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) work = false;
    if (work) {
        u32* l = lds + wave * 2048u;
        const u64 base = (u64)nb << 16;
        const u32 lim = size_hi - base >= 65536ull ? 65536u : (u32)(size_hi - base);    // (nb < col_to: base < size_hi)
        Blk D, A, B;
        blk_fill(D, 0u);
        bool covered = false;
        for (u32 i = 0; i < nplanes && !covered; ++i) {
            u64 da = mm_desc(descs, nblk, i, nb), db = mm_desc(descs, nblk, nplanes + i, nb);
            if (da == db) continue;                                  // both NULL, both FULL, or the same block: A ^ B = 0, nothing read
            if (DESC_K(da) == K_NULL) { blk_from_desc(db, B, l, lane); blk_or(D, B); }
            else if (DESC_K(db) == K_NULL) { blk_from_desc(da, A, l, lane); blk_or(D, A); }
            else {
                blk_from_desc(da, A, l, lane);
                blk_from_desc(db, B, l, lane);
#pragma unroll
                for (int r = 0; r < 8; ++r) D.r[r] |= A.r[r] ^ B.r[r];
            }
            covered = blk_covers_rows(D, lim, lane);
        }
        if (size_lo != size_hi) {                                    // rows only the longer column has (:716-731)
            blk_size_mask(A, nb, size_lo, lane);
            blk_size_mask(B, nb, size_hi, lane);
            blk_andn(B, A);
            blk_or(D, B);
        }
        if (null_mode != MM_NULL_NONE) {
            const bool has_a = uniform64((u64)(uintptr_t)descs[2u * nplanes]) != 0ull, has_b = uniform64((u64)(uintptr_t)descs[2u * nplanes + 1u]) != 0ull;
            const bool xr = null_mode == MM_NULL_OR_XOR;
            if (has_a || !xr) blk_from_desc(mm_desc(descs, nblk, 2u * nplanes, nb), A, l, lane);
            else blk_size_mask(A, nb, fill, lane);
            if (has_b || !xr) blk_from_desc(mm_desc(descs, nblk, 2u * nplanes + 1u, nb), B, l, lane);
            else blk_size_mask(B, nb, fill, lane);
            if (xr) { blk_xor(A, B); blk_or(D, A); }
            else { blk_or(A, B); blk_and(D, A); }
        }
        blk_size_mask(A, nb, size_hi, lane);
        blk_and(D, A);
        if (ending == MM_FIRST) {
            u32 mine = blk_first_bit(D, lane);
            if (lane == 0 && mine != 0xFFFFFFFFu)
                atomicMin(reinterpret_cast<unsigned long long*>(best), ((unsigned long long)nb << 16) + mine);
        } else {
            bool zero = blk_is_zero(D);
            if (ending == MM_COUNT) { if (!zero) cnt = wave_sum(blk_lane_popcount(D)); }
            else if (zero) store_trivial(K_NULL, nb, desc, st, lane);
            else store_result(D, nb, 1, slab, desc, st, lane);
        }
    }
    if (ending == MM_COUNT) count_fanin(cnt, slots, lane, wave);
}
