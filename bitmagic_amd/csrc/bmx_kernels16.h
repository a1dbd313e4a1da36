// bmx_kernels16.h -- pipeline results as index lists: the hits of EVERY arg-group of a pipeline as ascending positions, all groups
// in one CSR (aggregator::combine_and_sub(BII bi, ...) src/bmaggregator.h:1226-1284 per group; sparse_vector_scanner::find_eq(sv,
// value, bi) src/bmsparsevec_algo.h:1096 per value).  gfx950, wave64.
//
// Work items are the (column, group) items of k_pipe_counts (bmx_kernels.h), one wave each, read from the sorted descriptor matrix
// every pipeline carries (k_pipe_sort).  Three steps over a chunk of arg-groups:
//
//   k_pipe_hit_counts   evaluates the item exactly as k_pipe_counts does (pipe_chain over the bit-block operands, gap_apply_list in
//                       the wave's 8 KiB of LDS, the same early exits) and writes the ones of its result block into a table
//                       cnt[group][column] (u32, zeroed beforehand) instead of adding them to counts[group]
//   k_pipe_hit_scan     a workgroup per group: the group's row of cnt as u64 exclusive start positions, and the group's total
//   k_pipe_hit_offsets  one workgroup: the group totals of the WHOLE pipeline as the CSR offsets (u64: a group over vectors beyond
//                       2^32 bits can hold more than 2^32 hits)
//   k_pipe_hit_emit     the same items again: an item whose cnt is 0 leaves after the table read, every other one computes its
//                       block a second time and writes its positions at out[offsets[group] + start[group][column] ...]
//
// The block is computed twice on purpose.  Search groups die after a few operands (most items leave at an early exit and are
// never emitted), and keeping the result blocks between the passes would take items x 8 KiB; the table takes 12 B per item.
#pragma once
#include "bmx_kernels15.h"

// The result block of one (column, group) item whose row is neither ROW_EMPTY nor ROW_FULL: evaluation order and early exits of
// k_pipe_counts.  False: the block is all-zero (acc is then undefined).
template <int U>
__device__ __forceinline__ bool pipe_item_block(const u64* __restrict__ row, u64 hdr, u32 na, u32 ns, u32* lds, Blk& acc, u32 lane)
{
    const u32 nba = (u32)(hdr & 0xFFFFu), nga = (u32)((hdr >> 16) & 0xFFFFu);
    const u32 nbs = (u32)((hdr >> 32) & 0xFFFFu), ngs = (u32)(hdr >> 48);
    const u64* pa = row + 2;
    const u64* ps = pa + na;
    blk_fill(acc, ~0u);
    if (pipe_chain<U, true, 0>(acc, pa, nba, lane)) return false;
    if (pipe_chain<U, true, 1>(acc, ps, nbs, lane)) return false;
    if (nga | ngs) {
        blk_to_lds(acc, lds, lane);
        if (nga && gap_apply_list<GAP_AND>(pa + na - 1u, nga, lds, lane)) return false;
        if (ngs && gap_apply_list<GAP_SUB>(ps + ns - 1u, ngs, lds, lane)) return false;
        blk_from_lds(acc, lds, lane);
    }
    return true;
}

// row_off / and_n / sub_n: the tables of the chunk's groups (the pipeline's, advanced to the chunk's first group); ngroups = groups
// of the chunk; item = column * ngroups + group as in k_pipe_counts (neighbouring waves share a column's operand blocks);
// cnt[group * ncw + column], ncw = columns of the run
template <int U>
__global__ __launch_bounds__(256)
void k_pipe_hit_counts(const u64* __restrict__ dmat, const u32* __restrict__ row_off,
                       const u32* __restrict__ and_n, const u32* __restrict__ sub_n, u32 col_stride,
                       u32 ngroups, u32 col_from, u32 ncw, u32 nitems, int xcd_swz, u32* __restrict__ cnt)
{
    extern __shared__ u32 lds_dyn[];
    u32 lane = lane_id(), wave = threadIdx.x >> 6;
    u32 bid = xcd_swz ? xcd_remap(blockIdx.x, gridDim.x) : blockIdx.x;
    u32 item = uniform32(bid * 4u + wave);
    if (item >= nitems) return;
    u32 c = item / ngroups, g = item - c * ngroups;
    const u64* row = dmat + (size_t)(col_from + c) * col_stride + row_off[g];
    u64 hdr = uniform64(row[0]), flags = uniform64(row[1]);
    if (flags & ROW_EMPTY) return;
    u32 n = 65536u;
    if (!(flags & ROW_FULL)) {
        Blk acc;
        if (!pipe_item_block<U>(row, hdr, uniform32(and_n[g]), uniform32(sub_n[g]), lds_dyn + wave * 2048u, acc, lane)) return;
        n = wave_sum(blk_lane_popcount(acc));
    }
    if (lane == 0 && n) cnt[(size_t)g * ncw + c] = n;
}

// one workgroup per group of the chunk: start[g][c] = ones of the group in the columns before c (of this run), tot[g] = all of them
// (tot may be null: the totals are known already).  A pass covers 256 columns = at most 2^24 ones: u32 partials are exact.
__global__ __launch_bounds__(256)
void k_pipe_hit_scan(const u32* __restrict__ cnt, u32 ncw, u64* __restrict__ start, u64* __restrict__ tot)
{
    __shared__ u32 sm[4];
    const u32 tid = threadIdx.x, lane = tid & 63u, w = tid >> 6, g = blockIdx.x;
    const u32* row = cnt + (size_t)g * ncw;
    u64* srow = start + (size_t)g * ncw;
    u64 carry = 0;
    for (u64 base = 0; base < ncw; base += 256u) {
        const u64 c = base + tid;
        const u32 v = c < ncw ? row[c] : 0u;
        const u32 incl = wave_scan_incl(v, lane);
        if (lane == 63u) sm[w] = incl;
        __syncthreads();
        u32 off = 0, t = 0;
#pragma unroll
        for (u32 i = 0; i < 4u; ++i) { u32 a = sm[i]; if (i < w) off += a; t += a; }
        __syncthreads();
        if (c < ncw) srow[c] = carry + off + (incl - v);
        carry += t;
    }
    if (tot && tid == 0) tot[g] = carry;
}

// one workgroup: offsets[g] = hits of the groups before g, offsets[ngroups] = *total = all hits
__global__ __launch_bounds__(256)
void k_pipe_hit_offsets(const u64* __restrict__ tot, u32 ngroups, u64* __restrict__ offsets, u64* __restrict__ total)
{
    __shared__ u64 sm[4];
    const u32 tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    u64 carry = 0;
    for (u32 base = 0; base < ngroups; base += 256u) {
        const u32 g = base + tid;
        const u64 v = g < ngroups ? tot[g] : 0ull;
        u64 incl = v;
#pragma unroll
        for (u32 o = 1; o < 64u; o <<= 1) { u64 t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
        if (lane == 63u) sm[w] = incl;
        __syncthreads();
        u64 off = 0, t = 0;
#pragma unroll
        for (u32 i = 0; i < 4u; ++i) { u64 a = sm[i]; if (i < w) off += a; t += a; }
        __syncthreads();
        if (g < ngroups) offsets[g] = carry + off + (incl - v);
        carry += t;
    }
    if (tid == 0) { offsets[ngroups] = carry; *total = carry; }
}

// the positions of the ones of a block held in registers, ascending, at out[first ...]: per 256-word row a wave scan of the lanes'
// popcounts, then every lane writes the bits of its four words (the emit loop of k_expand_indices, bmx_kernels6.h)
template <typename T>
__device__ __forceinline__ void emit_block_bits(const Blk& b, u64 bit0, T* __restrict__ out, u64 first, u32 lane)
{
    u64 row_off = first;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        u32 c = (u32)__popc(b.r[i].x) + (u32)__popc(b.r[i].y) + (u32)__popc(b.r[i].z) + (u32)__popc(b.r[i].w);
        u32 incl = wave_scan_incl(c, lane);
        u32 tot = uniform32(__shfl(incl, 63, 64));
        u64 off = row_off + (incl - c);
        u64 wb = bit0 + ((u64)((u32)i * 256u + lane * 4u) << 5);
        emit_word_bits<T>(b.r[i].x, wb, out, off);
        emit_word_bits<T>(b.r[i].y, wb + 32u, out, off);
        emit_word_bits<T>(b.r[i].z, wb + 64u, out, off);
        emit_word_bits<T>(b.r[i].w, wb + 96u, out, off);
        row_off += tot;
    }
}

// T = u32 / u64 positions (absolute: column col_from + c starts at bit (col_from + c) << 16).  offsets: the CSR offsets advanced to
// the chunk's first group.  total = entries of out (the host has checked it against the caller's capacity): an item whose
// segment would not fit writes nothing.
template <int U, typename T>
__global__ __launch_bounds__(256)
void k_pipe_hit_emit(const u64* __restrict__ dmat, const u32* __restrict__ row_off,
                     const u32* __restrict__ and_n, const u32* __restrict__ sub_n, u32 col_stride,
                     u32 ngroups, u32 col_from, u32 ncw, u32 nitems, int xcd_swz, const u32* __restrict__ cnt,
                     const u64* __restrict__ start, const u64* __restrict__ offsets, T* __restrict__ out, u64 total)
{
    extern __shared__ u32 lds_dyn[];
    u32 lane = lane_id(), wave = threadIdx.x >> 6;
    u32 bid = xcd_swz ? xcd_remap(blockIdx.x, gridDim.x) : blockIdx.x;
    u32 item = uniform32(bid * 4u + wave);
    if (item >= nitems) return;
    u32 c = item / ngroups, g = item - c * ngroups;
    const u32 n = uniform32(cnt[(size_t)g * ncw + c]);
    if (!n) return;
    const u64 first = uniform64(offsets[g]) + uniform64(start[(size_t)g * ncw + c]);
    if (first + n > total) return;
    const u64 bit0 = (u64)(col_from + c) << 16;
    const u64* row = dmat + (size_t)(col_from + c) * col_stride + row_off[g];
    u64 hdr = uniform64(row[0]), flags = uniform64(row[1]);
    if (flags & ROW_FULL) {
        for (u32 i = lane; i < 65536u; i += 64u) out[first + i] = (T)(bit0 + i);
        return;
    }
    Blk acc;
    if (!pipe_item_block<U>(row, hdr, uniform32(and_n[g]), uniform32(sub_n[g]), lds_dyn + wave * 2048u, acc, lane)) return;
    emit_block_bits<T>(acc, bit0, out, first, lane);
}
