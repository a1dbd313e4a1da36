// bmx_kernels20.h -- batched equality search with WIDE keys over the bit planes of a resident column: the string half of
// sparse_vector_scanner (find_eq_str over bm::str_sparse_vector<>, src/bmsparsevec_algo.h:1194-1235, 3263-3436; planes are
// numbered octet * 8 + bit, src/bmstrsparsevec.h:1423).  gfx950, wave64.
#pragma once
#include "bmx_kernels19.h"

// ---------------------------------------------------------------------------
// k_slice_eq_keys: for n keys of T = ceil(P / 32) words at once, how many rows equal each key and which row is the first.
// The reference answers every string with its own AND-SUB group over the planes (prepare_and_sub_aggregator, :2546-2588);
// k_slice_eq_counts (bmx_kernels4.h) reads every plane block once whatever the number of queries, but holds a row's value
// in ONE register: 32 planes.  This is its wide form.
//   * work item = (block column, 4 of its 32 steps); a wave takes items from a persistent grid.  It resolves the plane
//     blocks of the column once per item into a per-wave LDS array (beyond ~32 planes the bases do not fit scalar registers):
//     0 = zeros (absent plane, NULL block, past the plane's end), 1 = ones (FULL), else the address of 8 KiB of raw bits --
//     a bit-block, or the plane's expanded window (GAP-holding planes are expanded by the host window by window, raw != null).
//   * step k loads word k * 64 + lane of every plane block (256 B per wave load, 4-byte nontemporal loads), 32 planes = one
//     32 x 32 bit tile at a time (bit_transpose32), and folds the row's word of every tile into a 32-bit fingerprint per row
//     (32 rows per lane).  A tile that is zero across the wave skips the butterfly.  The host folds the same T words per key.
//   * lookup as k_slice_eq_counts_big: presence filter, survivors compacted with ballots into a per-wave LDS queue (eight
//     rows of every lane at a time: at most 512 entries), probed 64 at a time against the open-addressing table
//     {fingerprint -> slot}.
//   * a fingerprint hit is only a candidate.  Each candidate (one per lane) gathers its row's T words out of the plane words
//     that were just loaded (P 4-byte loads, L2 hits; as bmx_kernels19.h picks a row's bits) into T words of per-wave LDS and
//     compares them with the T words of every slot of the probe chain whose fingerprint matches.  Keys are distinct: the walk
//     ends at the first equal key.  So the answer is exact whatever the fold does (fp_mask keeps only some fingerprint bits:
//     the test hook that makes verification decide nearly every row).
//   * verified hits: LDS count and LDS minimum per slot, flushed with one 64-bit global atomic add / min per slot and
//     workgroup.
// The all-zero key is not handled here (a row of zeros is NULL or the empty string: the host routes it through the aggregator).
// ---------------------------------------------------------------------------
struct EqkPlane { const u64* desc; const uint4* raw; u32 nblk; u32 pad_; };

#define EQK_EMPTY 0xFFFFFFFFu
#define EQK_FBITS 17u                   // presence filter: 128 Kbit = 16 KiB
#define EQK_QSZ 512u                    // queue entries per wave: 8 rows x 64 lanes
#define EQK_PARTS 8u                    // work items per block column (4 steps of 2,048 rows each)
#define EQK_SLOTS(nk) ((((nk) * 3u / 2u) + 64u) & ~63u)      // 1.5 slots per key, at least one empty

__host__ __device__ __forceinline__ u32 eqk_fold(u32 h, u32 w) { return (((h << 5) | (h >> 27)) ^ w) * 0x9E3779B1u; }
__host__ __device__ __forceinline__ u32 eqk_finish(u32 h, u32 mask) { h ^= h >> 15; h &= mask; return h == EQK_EMPTY ? 0xFFFFFFFEu : h; }
__host__ __device__ __forceinline__ u32 eqk_home(u32 fp, u32 tab) { return (u32)(((u64)(u32)(fp * 0x9E3779B1u) * tab) >> 32); }

// dynamic LDS of a workgroup of nw waves (bytes); the kernel lays it out in this order
__host__ __device__ __forceinline__ size_t eqk_lds_bytes(u32 tab, u32 T, u32 nw)
{
    return (size_t)tab * 8u /* first */ + (size_t)nw * T * 32u * 8u /* bases */ + (size_t)tab * 8u /* fp, count */
         + (1u << (EQK_FBITS - 3u)) + (size_t)nw * EQK_QSZ * 4u /* queue: fp */ + (size_t)nw * T * 64u * 4u /* row words */
         + (size_t)nw * EQK_QSZ * 2u /* queue: row */;
}

__global__ __launch_bounds__(512)
void k_slice_eq_keys(const EqkPlane* __restrict__ planes, u32 nplanes, u32 T, u32 c0, u32 c1, u64 size,
                     const u32* __restrict__ g_fp /* tab */, const u32* __restrict__ g_keys /* tab x T */, u32 tab, u32 fp_mask,
                     u64* __restrict__ counts /* per slot */, u64* __restrict__ first /* per slot, ~0 = none */)
{
    extern __shared__ u64 lds_eqk[];
    const u32 nw = blockDim.x >> 6, ppad = T * 32u;
    constexpr u32 FW = 1u << (EQK_FBITS - 5u);
    u64* fmin = lds_eqk;                                            // tab: lowest verified row per slot
    u64* bases = fmin + tab;                                        // nw x ppad
    u32* tfp = reinterpret_cast<u32*>(bases + (size_t)nw * ppad);   // tab fingerprints (EQK_EMPTY = free)
    u32* cnt = tfp + tab;                                           // tab counters
    u32* filt = cnt + tab;                                          // presence filter
    u32* qfp = filt + FW;                                           // nw x EQK_QSZ
    u32* rws = qfp + nw * EQK_QSZ;                                  // nw x T x 64: a candidate's row, word t of lane l at [t * 64 + l]
    u16* qrow = reinterpret_cast<u16*>(rws + nw * T * 64u);         // nw x EQK_QSZ: bit << 6 | lane
    for (u32 i = threadIdx.x; i < FW; i += blockDim.x) filt[i] = 0u;
    for (u32 i = threadIdx.x; i < tab; i += blockDim.x) { cnt[i] = 0u; fmin[i] = ~0ull; }
    __syncthreads();
    for (u32 i = threadIdx.x; i < tab; i += blockDim.x) {
        u32 f = g_fp[i];
        tfp[i] = f;
        if (f != EQK_EMPTY) { u32 hb = (f * 0x85EBCA6Bu) >> (32u - EQK_FBITS); atomicOr(&filt[hb >> 5], 1u << (hb & 31u)); }
    }
    __syncthreads();
    const u32 lane = lane_id(), wave = threadIdx.x >> 6;
    u64* myb = bases + (size_t)wave * ppad;
    u32* myqf = qfp + wave * EQK_QSZ;
    u16* myqr = qrow + wave * EQK_QSZ;
    u32* myrw = rws + wave * T * 64u;
    const u32 nitems = (c1 - c0) * EQK_PARTS;
    for (u32 it = uniform32(blockIdx.x * nw + wave); it < nitems; it += gridDim.x * nw) {
        const u32 c = c0 + it / EQK_PARTS, k0 = (it % EQK_PARTS) * (32u / EQK_PARTS);
        const u64 row0 = (u64)c << 16;
        const u32 lim = size <= row0 ? 0u : (size - row0 >= 65536ull ? 65536u : (u32)(size - row0));
        if (lim <= k0 * 2048u) continue;                            // (wave-uniform) the item lies past the column's end
        for (u32 p = lane; p < ppad; p += 64u) {
            u64 b = 0ull;
            if (p < nplanes) {
                const EqkPlane pl = planes[p];
                if (pl.raw) b = (u64)(uintptr_t)(pl.raw + (size_t)(c - c0) * 512u);
                else if (pl.desc && c < pl.nblk) {
                    u64 d = pl.desc[c];
                    b = DESC_K(d) == K_BIT ? DESC_P(d) : (DESC_K(d) == K_FULL ? 1ull : 0ull);
                }
            }
            myb[p] = b;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll 1
        for (u32 k = k0; k < k0 + 32u / EQK_PARTS; ++k) {
            const u32 wb = ((k * 64u + lane) << 5);                 // first row of this lane's word inside the block
            const u32 vm = lim >= wb + 32u ? ~0u : (lim <= wb ? 0u : ((1u << (lim - wb)) - 1u));
            u32 fp[32];
#pragma unroll
            for (int r = 0; r < 32; ++r) fp[r] = 0u;
            u32 any = 0u;
#pragma unroll 1
            for (u32 t = 0; t < T; ++t) {
                u32 a[32];
                u32 tany = 0u;
#pragma unroll
                for (int p = 0; p < 32; ++p) {
                    const u64 b = uniform64(myb[t * 32u + (u32)p]);
                    if (b > 1ull) a[p] = __builtin_nontemporal_load((const __attribute__((address_space(1))) u32*)(uintptr_t)b + k * 64u + lane);
                    else a[p] = b ? ~0u : 0u;
                    tany |= a[p];
                }
                any |= tany;
                if (__ballot(tany != 0u) == 0ull) {                 // 2,048 rows x 32 planes of zeros: the fold of a zero word
#pragma unroll
                    for (int r = 0; r < 32; ++r) fp[r] = eqk_fold(fp[r], 0u);
                    continue;
                }
                bit_transpose32(a);
#pragma unroll
                for (int r = 0; r < 32; ++r) fp[r] = eqk_fold(fp[r], a[r]);
            }
            if (__ballot((any & vm) != 0u) == 0ull) continue;       // no row of the step holds a bit: no non-zero key matches
#pragma unroll
            for (int r = 0; r < 32; ++r) fp[r] = eqk_finish(fp[r], fp_mask);
#pragma unroll
            for (int r0 = 0; r0 < 32; r0 += 8) {
                u32 f[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) { u32 hb = (fp[r0 + j] * 0x85EBCA6Bu) >> (32u - EQK_FBITS); f[j] = filt[hb >> 5] >> (hb & 31u); }
                u32 nq = 0;                                         // survivors of these 512 rows (wave-uniform)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int r = r0 + j;
                    bool hit = (f[j] & 1u) && ((vm >> r) & 1u);
                    u64 m = __ballot(hit);
                    if (m) {
                        u32 pos = nq + __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u));
                        if (hit) { myqf[pos] = fp[r]; myqr[pos] = (u16)(((u32)r << 6) | lane); }
                        nq += (u32)__popcll(m);
                    }
                }
                if (!nq) continue;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                for (u32 b0 = 0; b0 < nq; b0 += 64u) {
                    const bool act = b0 + lane < nq;
                    const u32 v = act ? myqf[b0 + lane] : 0u, rid = act ? (u32)myqr[b0 + lane] : 0u;
                    const u32 cl = rid & 63u, cr = rid >> 6;        // the candidate row: bit cr of word k * 64 + cl
#pragma unroll 1
                    for (u32 t = 0; t < T; ++t) {
                        u32 w = 0u;
#pragma unroll 8
                        for (u32 p = 0; p < 32u; ++p) {
                            const u64 b = uniform64(myb[t * 32u + p]);
                            u32 x;
                            if (b > 1ull) x = *((const u32*)(uintptr_t)b + k * 64u + cl);
                            else x = b ? ~0u : 0u;
                            w |= ((x >> cr) & 1u) << p;
                        }
                        myrw[t * 64u + lane] = w;                   // (written and read by this lane only)
                    }
                    if (act) {
                        u32 h = eqk_home(v, tab);
                        for (;;) {
                            const u32 kk = tfp[h];
                            if (kk == EQK_EMPTY) break;
                            if (kk == v) {
                                bool eq = true;
                                for (u32 t = 0; t < T && eq; ++t) eq = g_keys[(size_t)h * T + t] == myrw[t * 64u + lane];
                                if (eq) {
                                    atomicAdd(&cnt[h], 1u);
                                    atomicMin(reinterpret_cast<unsigned long long*>(&fmin[h]), (unsigned long long)(row0 + ((k * 64u + cl) << 5) + cr));
                                    break;
                                }
                            }
                            h = h + 1u == tab ? 0u : h + 1u;
                        }
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    __syncthreads();
    for (u32 i = threadIdx.x; i < tab; i += blockDim.x)
        if (cnt[i]) {
            atomicAdd(reinterpret_cast<unsigned long long*>(&counts[i]), (unsigned long long)cnt[i]);
            atomicMin(reinterpret_cast<unsigned long long*>(&first[i]), (unsigned long long)fmin[i]);
        }
}
