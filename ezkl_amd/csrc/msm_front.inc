// msm_front.inc -- the two passes of the MSM's sort front end that recode scalars (histogram, partition), included TWICE by msm.hip:
//   MSM_ONCE 0   msm_hist_kernel, msm_partition_kernel: the fixed-base chain.  Every pair is kept; the text below is then, token for
//                token, what these kernels were before the table-free path existed, and so is their code;
//   MSM_ONCE 1   msm_hist_once_kernel, msm_partition_once_kernel (+ a last argument w0): the MSM without window tables (msm_once_run).
//                Member blockIdx.z of a fused group is ONE window, w0 + blockIdx.z, of the same scalar column, and only that window's
//                pairs are kept; the caller passes tab_stride = 0 and base_offset = 0, so a payload is the point's index.
// Two kernels per pass and not one with a run-time switch or a shared body behind two wrappers: the first costs the fixed-base chain a
// test per digit, the second compiled msm_partition_kernel to different code (the body, optimised apart from its kernel, lost the
// kernel's workgroup-size facts).  Not a template: the chain's kernels are looked up by their plain names (tests/test_msm_isa_cpu.py).
#if MSM_ONCE
#define MSM_HIST_KERNEL msm_hist_once_kernel
#define MSM_PARTITION_KERNEL msm_partition_once_kernel
#define MSM_ONCE_PARAM , uint32_t w0
#define MSM_KEEP(w) ((w) == w0 + blockIdx.z)
#else
#define MSM_HIST_KERNEL msm_hist_kernel
#define MSM_PARTITION_KERNEL msm_partition_kernel
#define MSM_ONCE_PARAM
#define MSM_KEEP(w) true
#endif
__global__ __launch_bounds__(256) void MSM_HIST_KERNEL(MsmCols cols, size_t n, size_t per_block, WinPlan wp,
                                                       uint32_t LB, uint32_t NP, uint32_t* wg_hist,
                                                       uint32_t* zero_base, uint32_t zero_words, size_t bstride MSM_ONCE_PARAM) {
    BOFF(); BSH(wg_hist);
    const fe_t* scalars = msm_col(cols);
    if (zero_base) {                                                      // the chain's counters, bin totals and planes start at zero
        BSH(zero_base);
        for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < zero_words; i += gridDim.x * 256) zero_base[i] = 0;
    }
    __shared__ uint32_t lh[(1u << MSM_MAX_PART_BITS) + 1];
    const uint32_t NQ = NP + 1;                                           // + the bucket-0 partition
    for (uint32_t p = threadIdx.x; p < NQ; p += 256) lh[p] = 0;
    __syncthreads();
    size_t lo = (size_t)blockIdx.x * per_block, hi = lo + per_block < n ? lo + per_block : n;
    for (size_t i0 = lo + threadIdx.x; i0 < hi; i0 += 4 * 256) {
        // four scalars per thread: their eight 16-byte loads are all issued here, ahead of the first reduction (which is inlined arithmetic,
        // so the compiler waits for each scalar with a counted vmcnt and the other loads stay in flight): one HBM round trip per thread
        fe_t s[4];
        uint32_t neg[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const size_t i = i0 + (size_t)q * 256;
            s[q] = i < hi ? ld_fe(scalars + i) : Fr::zero();
        }
#pragma unroll
        for (int q = 0; q < 4; q++) s[q] = msm_canon(s[q], neg[q]);
        msm_recode<4>(s, neg, wp, [&](int, uint32_t w, uint32_t bucket, uint32_t) { if (MSM_KEEP(w)) atomicAdd(&lh[msm_part_of(bucket, NP)], 1u); });
    }
    __syncthreads();
    // row of this workgroup, coalesced; wg_hist is scanned in place later (the partition pass takes the raw counts back as row differences)
    for (uint32_t p = threadIdx.x; p < NQ; p += 256) wg_hist[(size_t)blockIdx.x * NQ + p] = lh[p];
}
__global__ __launch_bounds__(1024) void MSM_PARTITION_KERNEL(MsmCols cols, size_t n, size_t per_block, uint32_t G, WinPlan wp,
                                                             uint32_t LB, uint32_t NP, size_t base_offset, size_t tab_stride,
                                                             const uint32_t* part_base, const uint32_t* wg_hist, const uint32_t* part_count, uint2* entries,
                                                             uint32_t* vals, size_t bstride MSM_ONCE_PARAM) {
    BOFF(); BSH(part_base); BSH(wg_hist); BSH(part_count); BSH(entries); BSH(vals);
    const fe_t* scalars = msm_col(cols);
    extern __shared__ uint32_t plds[];
    __shared__ uint32_t tsum[1024];
    const uint32_t NQ = NP + 1;                // partitions incl. bucket 0's (msm_part_of); the arrays below are padded to NQ + 1 words
    uint32_t* start = plds;                    // NQ: first staged index of partition p
    uint32_t* cursor = plds + (NQ + 1);        // NQ: next free staged index
    uint32_t* gbase = plds + 2 * (NQ + 1);     // NQ: global slot of the workgroup's first pair of partition p
    uint2* stage = reinterpret_cast<uint2*>(plds + 3 * (NQ + 1));
    const uint32_t t = threadIdx.x, T = blockDim.x;
    const uint32_t K = (NQ + T - 1) / T;       // consecutive partitions per thread
    const uint32_t PB = 31 - __clz(NP);
    // scanned count of (tile, p) and of the row after it
    auto row = [&](uint32_t tile, uint32_t p) { return wg_hist[(size_t)tile * NQ + p]; };
    auto row_next = [&](uint32_t tile, uint32_t p) { return tile + 1 < G ? wg_hist[(size_t)(tile + 1) * NQ + p] : part_count[p]; };
    fe_t sm[1];
    uint32_t h0[MSM_PART_PF], h1[MSM_PART_PF];
    auto fetch = [&](uint32_t tile) {
        const size_t lo = (size_t)tile * per_block, hi = lo + per_block < n ? lo + per_block : n;
        sm[0] = lo + t < hi ? ld_fe(scalars + lo + t) : Fr::zero();
#pragma unroll
        for (uint32_t q = 0; q < MSM_PART_PF; q++) {
            const uint32_t p = t * K + q;
            const bool in = q < K && p < NQ;
            h0[q] = in ? row(tile, p) : 0u;
            h1[q] = in ? row_next(tile, p) : 0u;
        }
    };
    if (blockIdx.x < G) fetch(blockIdx.x);
    for (uint32_t tile = blockIdx.x; tile < G; tile += gridDim.x) {
        // exclusive scan of the tile's raw counts: K consecutive partitions per thread, then a scan over threads (its first barrier also
        // ends the previous tile's write-out before start / cursor / gbase / stage are written again)
        uint32_t loc = 0;
#pragma unroll
        for (uint32_t q = 0; q < MSM_PART_PF; q++) loc += h1[q] - h0[q];
        for (uint32_t q = MSM_PART_PF; q < K; q++) {
            const uint32_t p = t * K + q;
            if (p < NQ) loc += row_next(tile, p) - row(tile, p);
        }
        uint32_t total;
        uint32_t run = msm_block_scan(loc, tsum, total) - loc;
#pragma unroll
        for (uint32_t q = 0; q < MSM_PART_PF; q++) {
            const uint32_t p = t * K + q;
            if (q < K && p < NQ) {
                start[p] = run;
                cursor[p] = run;
                gbase[p] = part_base[p] + h0[q];
                run += h1[q] - h0[q];
            }
        }
        for (uint32_t q = MSM_PART_PF; q < K; q++) {
            const uint32_t p = t * K + q;
            if (p < NQ) {
                const uint32_t r0 = row(tile, p);
                start[p] = run;
                cursor[p] = run;
                gbase[p] = part_base[p] + r0;
                run += row_next(tile, p) - r0;
            }
        }
        __syncthreads();
        const size_t lo = (size_t)tile * per_block, hi = lo + per_block < n ? lo + per_block : n;
        const size_t i = lo + t;
        if (i < hi) {
            uint32_t neg[1];
            sm[0] = msm_canon(sm[0], neg[0]);
            msm_recode<1>(sm, neg, wp, [&](int, uint32_t w, uint32_t bucket, uint32_t sign) {
                if (!MSM_KEEP(w)) return;
                const uint32_t r = atomicAdd(&cursor[msm_part_of(bucket, NP)], 1u);
                stage[r] = make_uint2((uint32_t)(w * tab_stride + base_offset + i) | (sign << 31), bucket);
            });
        }
        __syncthreads();
        if (tile + gridDim.x < G) fetch(tile + gridDim.x);     // the next tile's loads travel under this tile's write-out
        for (uint32_t idx = t; idx < total; idx += T) {
            const uint2 e = stage[idx];
            const uint32_t p = msm_part_of(e.y, NP);
            const uint32_t slot = gbase[p] + (idx - start[p]);
            if (p) entries[slot] = make_uint2(e.x, e.y >> PB);
            else vals[slot] = e.x;                              // bucket 0: already in its final place (its partition comes first)
        }
    }
}
#undef MSM_HIST_KERNEL
#undef MSM_PARTITION_KERNEL
#undef MSM_ONCE_PARAM
#undef MSM_KEEP
