// bmx_kernels19.h -- the values of the selected rows of a resident bit-sliced column, read out of the planes: what
// set2set_11_transform::remap gathers per window (src/bmsparsevec_algo.h:2114-2205: enumerate bv_in & not_null, sv.gather, bv_out.set)
// as one list on the device (bmx_slice_values / bmx_slice_remap).  gfx950, wave64.
#pragma once
#include "bmx_kernels18.h"

// ---------------------------------------------------------------------------
// Operand table (operand_list / direct_table): rows [0, P) the planes, row P the not-NULL vector, row P + 1 the selector
// bv_in; a null row is a plane / vector that does not exist (absent not-NULL vector or selector = all ones); a row that ends
// before block column nb reads as zeros there.  A wave owns block column nb of the row space:
//     S = bv_in[nb] & not_null[nb] & ones[0, size)                       any block kind (blk_from_desc)
//   k_slice_sel_counts  cnt[nb] = popcount(S)
//   k_pipe_hit_scan     (bmx_kernels16.h, one group) the exclusive starts of the columns and the total n
//   k_slice_values      a column whose cnt is 0 leaves after the table read: no plane is touched.  Otherwise S again, the row
//                       ids (optional) through emit_block_bits, and the values by the formulation below.
// Emit formulation (C = SV_PASS = 2048): the selected rows of the column are taken in passes of C; the in-block positions of
// a pass go to LDS as u16 in ascending order (per 256-word row of S a wave scan of the lanes'
// popcounts, every lane writes the bits of its four words); lane l then owns rows k = l + 64 t of the pass, t < C / 64 = 32,
// keeps their positions and their values in registers (32 accumulators, 64 at width 8), and the planes are the OUTER loop: a
// plane block goes through blk_from_desc into the wave's 8 KiB LDS stage (blk_to_lds) and every lane picks the bits of its
// rows from there.  A NULL plane block is skipped, a FULL one ORs 1 << p into every row without a read.  A column with more
// than C selected rows repeats the plane loop per pass (the planes then come from L2): correct, not the tuned case.  The
// values leave as out[first + k], consecutive lanes to consecutive entries.
// LDS: per wave 8 KiB stage + 4 KiB positions, 48 KiB per workgroup of four waves: three workgroups fit the 160 KiB of a CU.
// ---------------------------------------------------------------------------
#define SV_PASS 2048u
#define SV_T 32            // SV_PASS / 64

// S of block column nb; false: S is all-zero (then undefined)
__device__ __forceinline__ bool sv_selected(const u64* const* __restrict__ descs, const u32* __restrict__ nblk, u32 P, u32 nb, u64 size,
                                            Blk& S, u32* l, u32 lane)
{
    const bool has_nn = uniform64((u64)(uintptr_t)descs[P]) != 0ull, has_sel = uniform64((u64)(uintptr_t)descs[P + 1u]) != 0ull;
    const u64 dn = has_nn ? mm_desc(descs, nblk, P, nb) : DESC_MAKE(0, K_FULL);
    const u64 ds = has_sel ? mm_desc(descs, nblk, P + 1u, nb) : DESC_MAKE(0, K_FULL);
    if (DESC_K(dn) == K_NULL || DESC_K(ds) == K_NULL) return false;
    blk_size_mask(S, nb, size, lane);
    Blk T;
    if (DESC_K(dn) != K_FULL) { blk_from_desc(dn, T, l, lane); blk_and(S, T); }
    if (DESC_K(ds) != K_FULL) { blk_from_desc(ds, T, l, lane); blk_and(S, T); }
    return true;
}

__global__ __launch_bounds__(256)
void k_slice_sel_counts(const u64* const* __restrict__ descs, const u32* __restrict__ nblk, u32 nplanes, u32 ncols, u64 size,
                        u32* __restrict__ cnt)
{
    __shared__ u32 lds[4 * 2048];
    const u32 lane = lane_id(), wave = threadIdx.x >> 6;
    const u32 nb = uniform32(blockIdx.x * 4u + wave);
    if (nb >= ncols) return;
    Blk S;
    u32 n = 0;
    if (sv_selected(descs, nblk, nplanes, nb, size, S, lds + wave * 2048u, lane)) n = wave_sum(blk_lane_popcount(S));
    if (lane == 0) cnt[nb] = n;
}

// in-block positions [k0, k0 + SV_PASS) of the ones of S, ascending, as pos[k - k0]
__device__ __forceinline__ void sv_pass_positions(const Blk& S, u32 k0, u16* pos, u32 lane)
{
    u32 row_off = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const u32 w[4] = {S.r[i].x, S.r[i].y, S.r[i].z, S.r[i].w};
        const u32 c = (u32)__popc(w[0]) + (u32)__popc(w[1]) + (u32)__popc(w[2]) + (u32)__popc(w[3]);
        const u32 incl = wave_scan_incl(c, lane);
        u32 k = row_off + (incl - c);
        row_off += uniform32(__shfl(incl, 63, 64));
        if (k + c <= k0 || k >= k0 + SV_PASS) continue;                 // (per lane: none of its rows is in the pass)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const u32 b0 = ((u32)i * 256u + lane * 4u + (u32)j) << 5;
            u32 x = w[j];
            while (x) {
                const u32 b = (u32)__builtin_ctz(x);
                if (k - k0 < SV_PASS) pos[k - k0] = (u16)(b0 + b);      // (k < k0 wraps beyond SV_PASS)
                ++k; x &= x - 1u;
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// W = 1: u32 values (P <= 32), W = 2: u64 values (P <= 64).  T = type of the row ids (u32 / u64), rows may be null.
// total = entries of values / rows (the host has checked it against the caller's capacity): a column whose segment would not
// fit writes nothing.
template <int W, typename T>
__global__ __launch_bounds__(256)
void k_slice_values(const u64* const* __restrict__ descs, const u32* __restrict__ nblk, u32 nplanes, u32 ncols, u64 size,
                    const u32* __restrict__ cnt, const u64* __restrict__ start, T* __restrict__ values, T* __restrict__ rows, u64 total)
{
    __shared__ u32 lds[4 * 2048];
    __shared__ u16 posl[4 * SV_PASS];
    const u32 lane = lane_id(), wave = threadIdx.x >> 6;
    const u32 nb = uniform32(blockIdx.x * 4u + wave);
    if (nb >= ncols) return;
    const u32 n = uniform32(cnt[nb]);
    if (!n) return;
    const u64 first = uniform64(start[nb]);
    if (n > 65536u || first + n > total) return;
    u32* l = lds + wave * 2048u;
    u16* pos = posl + wave * SV_PASS;
    Blk S;
    if (!sv_selected(descs, nblk, nplanes, nb, size, S, l, lane)) return;
    if (rows) emit_block_bits<T>(S, (u64)nb << 16, rows, first, lane);
    for (u32 k0 = 0; k0 < n; k0 += SV_PASS) {
        const u32 np = n - k0 < SV_PASS ? n - k0 : SV_PASS;             // rows of this pass
        sv_pass_positions(S, k0, pos, lane);
        u32 rp[SV_T], lo[SV_T], hi[W == 2 ? SV_T : 1];
#pragma unroll
        for (int t = 0; t < SV_T; ++t) {
            lo[t] = 0u; if (W == 2) hi[t] = 0u;
            rp[t] = (u32)t * 64u + lane < np ? (u32)pos[(u32)t * 64u + lane] : 0u;
        }
        for (u32 p = 0; p < nplanes; ++p) {
            const u64 d = mm_desc(descs, nblk, p, nb);
            const u32 k = DESC_K(d);
            if (k == K_NULL) continue;
            const u32 bit = 1u << (p & 31u);
            const bool low = W == 1 || p < 32u;
            if (k == K_FULL) {
#pragma unroll
                for (int t = 0; t < SV_T; ++t) { if (low) lo[t] |= bit; else if (W == 2) hi[t] |= bit; }
                continue;
            }
            Blk B;
            blk_from_desc(d, B, l, lane);
            blk_to_lds(B, l, lane);
#pragma unroll
            for (int t = 0; t < SV_T; ++t) {
                if ((u32)t * 64u < np) {                                // (wave-uniform)
                    const u32 m = ((l[rp[t] >> 5] >> (rp[t] & 31u)) & 1u) ? bit : 0u;
                    if (low) lo[t] |= m; else if (W == 2) hi[t] |= m;
                }
            }
            __builtin_amdgcn_wave_barrier();                            // (every lane has read the stage before the next plane fills it)
        }
#pragma unroll
        for (int t = 0; t < SV_T; ++t) {
            const u32 kk = (u32)t * 64u + lane;
            if (kk < np) values[first + k0 + kk] = W == 2 ? (T)(((u64)hi[W == 2 ? t : 0] << 32) | lo[t]) : (T)lo[t];
        }
    }
}
