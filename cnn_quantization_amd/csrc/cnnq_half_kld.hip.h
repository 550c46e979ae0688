// cnnq_half_kld.hip.h - the `-kld` histogram (kld_threshold.py:19-23: numpy.histogram(arr, 2001, range = (-th, th))) on bf16 /
// fp16 rows x[rows][len], read where they lie.
// Part of the single translation unit cnnq_kernels.hip (see its header for the design).
//
// The contract: hist is, count for count, k_kld_hist's on x.float().  The upconversion is exact (h_up), so
// every element is the double the fp32 kernel bins, and the binning is that kernel's own (kld_range, kld_count, kld_flush in
// cnnq_kld.hip.h): the same range, the same corrected index, `first <= a <= last` drops NaN, the same KREP replicas in LDS and the
// same flush of the non-zero counts.  Counts are integers, so the order in which a row's elements arrive changes nothing - which
// is also why a sample of a dense channels_last tensor, one contiguous block, is a row like any other.  k_kld_search / k_kld_pick
// see the histogram and the row extrema only: everything behind this kernel is the fp32 route's, bit for bit.
//
// Loads: a workgroup owns one chunk of KCHUNK elements of one row (k_kld_hist's grid).  It reads the chunk's first elements one
// by one up to the first 16-byte boundary, then eight elements per 16-byte load, then the rest - fewer than eight - one by one.
// The boundary is found from the chunk's own address, per workgroup: with an odd row length the rows after the first start
// misaligned, and a view may start at an odd element; both still get 16-byte loads for all but at most 14 elements of a chunk.
// Non-temporal like k_kld_hist's: the extrema pass in front has read x already and nothing reads it after.
#pragma once
#include "cnnq_half.hip.h"
#include "cnnq_kld.hip.h"

namespace {

constexpr int KHW = 8;   // elements of one 16-byte load

template <class T>
__global__ void __launch_bounds__(TPB) k_h_kld_hist(const uint16_t* __restrict__ x, int64_t len, const float* __restrict__ rowmm,
                                                    int rows, unsigned* __restrict__ hist) {
    __shared__ unsigned sh[KB * KREP];
    const int row = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < KB * KREP; i += TPB) sh[i] = 0;
    const KldRange r = kld_range(rowmm[row], rowmm[rows + row]);
    if (!r.ok) return;   // the whole workgroup: the row stays as the host zeroed it
    __syncthreads();
    const int64_t beg = (int64_t)blockIdx.x * KCHUNK;
    const int n = (int)(min(beg + (int64_t)KCHUNK, len) - beg);     // 1 .. KCHUNK elements of this row
    const uint16_t* __restrict__ p = x + (int64_t)row * len + beg;
    const int rep = tid & (KREP - 1);
    // [0, head): up to the 16-byte boundary (p is 2-byte aligned: 0 .. 7 elements); [head, head + nv * 8): whole loads; the tail
    const int head = min((int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 1), n);
    const int nv = (n - head) / KHW;
    const int tail = head + nv * KHW;
    if (tid < head) kld_count(r, h_up(T{}, p[tid]), sh, rep);
    for (int v = tid; v < nv; v += TPB) {
        uint16_t e[KHW];
        h_ld<KHW, true>(p + head + v * KHW, e);
#pragma unroll
        for (int k = 0; k < KHW; ++k) kld_count(r, h_up(T{}, e[k]), sh, rep);
    }
    if (tid < n - tail) kld_count(r, h_up(T{}, p[tail + tid]), sh, rep);
    __syncthreads();
    kld_flush(sh, hist + (size_t)row * KB);
}

}  // namespace
