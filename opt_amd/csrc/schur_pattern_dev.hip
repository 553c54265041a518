// schur_pattern_dev.hip — schur_pattern_build (schur_pattern.h) as sort-and-scan work on the
// device. The arrays equal the host builder's element for element:
//
//   instances    per list a stable sort by eliminated vertex gives the positions base_l + rank
//                (the plan hands in GenArgs::geid, which is that order); the lists' instances,
//                concatenated in that order and stably sorted by eliminated vertex once more,
//                stand per vertex in the order [list, position]: iq (position) and ir (retained
//                vertex). off[p] is a lower bound in the sorted vertices, no histogram.
//   pair counts  k_p^2 (k_p (k_p - 1) in the `distinct` form) per vertex, a 64-bit exclusive
//                scan, the total read back (read-back 1) and checked before anything of that
//                size is allocated.
//   enumeration  one thread per PAIR: pair t finds its vertex by bisection in the scanned
//                counts and its (x, y) by division, so a hub's 10^6 pairs spread over the grid
//                like everybody else's. Key row * 2^cb + col, value (q1, q2) packed in 8 bytes.
//   sort         one stable radix sort over bits [0, 2 cb): inside a block the pairs keep the
//                enumeration order, which the assembly kernels' summation order rests on. The
//                sorted values ARE the pairs array. 4-byte keys while 2 cb <= 32.
//   blocks       heads of the key runs (an order-preserving select) are the pair-bearing blocks
//                u; per row two bisections over them give its first block, its blocks left of
//                the diagonal and whether the diagonal bears pairs; rowPtr is the scan of
//                cnt + !hasDiag; the counts are read back (read-back 2), then every block and
//                every inserted diagonal is written to its place.
//   long lists   order-preserving selects over pairPtr / rowPtr.
//
// No atomic orders anything: the only atomics are the two integer counts of long blocks and long
// rows. Temporaries, K = 4 or 8 bytes per key:
//   24 nq + 12 (nE + 1) + [8 n_l per list sorted here] + (2 K + 8) np + 21 (nR + 1) + the sorts'
//   and selects' own scratch.
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <string>
#include "csr.h"
#include "schur_pattern_dev.h"

namespace optamd {

namespace {

constexpr int kB = 256;
constexpr long long kMaxInt = 2147483647LL;
typedef unsigned long long u64;

int grid_for(long long n) { return (int)std::max<long long>(1, std::min<long long>((n + kB - 1) / kB, 4096)); }

// first i in [lo, hi) with v[i] >= x (hi if none)
__device__ inline int lower_bound_int(const int* v, int lo, int hi, int x) {
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (v[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void sp_iota(int* v, long long n) {
    for (long long i = (long long)blockIdx.x * kB + threadIdx.x; i < n; i += (long long)gridDim.x * kB) v[i] = (int)i;
}
// one list's instances in list order: eliminated vertex, position, retained vertex
__global__ void sp_gather(const int* ev, const int* rv, const int* order, long long n, long long ebase, long long base,
                          int* K, int* V, int* R) {
    for (long long i = (long long)blockIdx.x * kB + threadIdx.x; i < n; i += (long long)gridDim.x * kB) {
        const int e = order ? order[i] : (int)i;
        K[base + i] = ev ? ev[e] : (int)(ebase + e);
        V[base + i] = (int)(base + i);
        R[base + i] = rv[e];
    }
}
__global__ void sp_gather_ir(const int* R, const int* iq, long long nq, int* ir) {
    for (long long i = (long long)blockIdx.x * kB + threadIdx.x; i < nq; i += (long long)gridDim.x * kB) ir[i] = R[iq[i]];
}
// off[p]: the first instance of vertex p in the sorted vertices Ks; w[p]: its pair count
__global__ void sp_offsets(const int* Ks, int nq, long long nE, int distinct, int* off, long long* w) {
    for (long long p = (long long)blockIdx.x * kB + threadIdx.x; p <= nE; p += (long long)gridDim.x * kB) {
        const int a = p < nE ? lower_bound_int(Ks, 0, nq, (int)p) : nq;
        const int b = p + 1 < nE ? lower_bound_int(Ks, a, nq, (int)(p + 1)) : nq;
        off[p] = a;
        const long long k = b - a;
        w[p] = p < nE ? (distinct ? k * (k - 1) : k * k) : 0;
    }
}
template <class K>
__global__ void sp_enumerate(const long long* poff, const int* off, const int* iq, const int* ir, long long nE,
                             long long np, int cb, int distinct, K* keys, u64* vals) {
    for (long long t = (long long)blockIdx.x * kB + threadIdx.x; t < np; t += (long long)gridDim.x * kB) {
        long long lo = 0, hi = nE;   // poff[lo] <= t < poff[hi]
        while (hi - lo > 1) {
            const long long mid = lo + (hi - lo) / 2;
            if (poff[mid] <= t) lo = mid; else hi = mid;
        }
        const int o = off[lo], k = off[lo + 1] - o;
        const unsigned local = (unsigned)(t - poff[lo]), div = (unsigned)(distinct ? k - 1 : k);
        const unsigned x = local / div;
        unsigned y = local - x * div;
        if (distinct && y >= x) ++y;
        keys[t] = ((K)(unsigned)ir[o + x] << cb) | (K)(unsigned)ir[o + y];
        vals[t] = (u64)(unsigned)iq[o + x] | ((u64)(unsigned)iq[o + y] << 32);
    }
}
template <class K>
struct IsHead {
    const K* key;
    __device__ bool operator()(int i) const { return i == 0 || key[i] != key[i - 1]; }
};
struct IsLong {
    const int* ptr;
    int limit;
    __device__ bool operator()(int i) const { return ptr[i + 1] - ptr[i] > limit; }
};
// first u in [lo, hi) whose block key is >= x
template <class K>
__device__ inline int lower_bound_block(const K* key, const int* ustart, int lo, int hi, u64 x) {
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if ((u64)key[ustart[mid]] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// per row: its first pair-bearing block, its blocks left of the diagonal, the diagonal's presence
template <class K>
__global__ void sp_rows(const K* key, const int* ustart, const int* nu_d, long long nR, int cb, int* first, int* lt,
                        unsigned char* hasDiag) {
    const int nu = *nu_d;
    for (long long r = (long long)blockIdx.x * kB + threadIdx.x; r <= nR; r += (long long)gridDim.x * kB) {
        if (r == nR) { first[r] = nu; continue; }
        const u64 rowkey = (u64)r << cb;
        const int f = lower_bound_block(key, ustart, 0, nu, rowkey);
        const int d = lower_bound_block(key, ustart, f, nu, rowkey | (u64)r);
        first[r] = f;
        lt[r] = d - f;
        hasDiag[r] = d < nu && (u64)key[ustart[d]] == (rowkey | (u64)r);
    }
}
__global__ void sp_row_counts(const int* first, const unsigned char* hasDiag, long long nR, long long* w) {
    for (long long r = (long long)blockIdx.x * kB + threadIdx.x; r <= nR; r += (long long)gridDim.x * kB)
        w[r] = r < nR ? (long long)(first[r + 1] - first[r]) + (hasDiag[r] ? 0 : 1) : 0;
}
// counts: {pair-bearing blocks, blocks, long blocks, long rows}; rowPtr from the 64-bit scan
__global__ void sp_counts(const long long* rp64, long long nR, const int* ustart, const int* nu_d, long long np,
                          int long_pairs, int long_row, int* rowPtr, u64* counts) {
    const int nu = *nu_d;
    const long long i0 = (long long)blockIdx.x * kB + threadIdx.x, stride = (long long)gridDim.x * kB;
    if (i0 == 0) { counts[0] = (u64)nu; counts[1] = (u64)rp64[nR]; }
    for (long long r = i0; r <= nR; r += stride) {
        rowPtr[r] = (int)rp64[r];
        if (long_row > 0 && r < nR && rp64[r + 1] - rp64[r] > long_row) atomicAdd(&counts[3], 1ULL);
    }
    for (long long u = i0; u < nu; u += stride) {
        const long long end = u + 1 < nu ? ustart[u + 1] : np;
        if (end - ustart[u] > long_pairs) atomicAdd(&counts[2], 1ULL);
    }
}
template <class K>
__global__ void sp_fill_blocks(const K* key, const int* ustart, const int* nu_d, int cb, const int* rowPtr,
                               const int* first, const unsigned char* hasDiag, int* colInd, int* blkRow, int* pairPtr) {
    const int nu = *nu_d;
    const u64 mask = (1ULL << cb) - 1;
    for (long long u = (long long)blockIdx.x * kB + threadIdx.x; u < nu; u += (long long)gridDim.x * kB) {
        const u64 k = (u64)key[ustart[u]];
        const int r = (int)(k >> cb), c = (int)(k & mask);
        const int pos = rowPtr[r] + (int)(u - first[r]) + ((!hasDiag[r] && c > r) ? 1 : 0);
        colInd[pos] = c;
        blkRow[pos] = r;
        pairPtr[pos] = ustart[u];
    }
}
// the diagonal blocks no pair lands on, with the empty list the host's open(r) writes
__global__ void sp_fill_diag(const int* ustart, const int* nu_d, long long np, long long nR, const int* rowPtr,
                             const int* first, const int* lt, const unsigned char* hasDiag, int* colInd, int* blkRow,
                             int* pairPtr) {
    const int nu = *nu_d;
    for (long long r = (long long)blockIdx.x * kB + threadIdx.x; r <= nR; r += (long long)gridDim.x * kB) {
        if (r == nR) { pairPtr[rowPtr[nR]] = (int)np; continue; }
        if (hasDiag[r]) continue;
        const int pos = rowPtr[r] + lt[r], next = first[r] + lt[r];
        colInd[pos] = (int)r;
        blkRow[pos] = (int)r;
        pairPtr[pos] = next < nu ? ustart[next] : (int)np;
    }
}

// temporaries: freed when the build ends, however it ends
struct Arena {
    std::vector<void*> ptrs;
    long long bytes = 0;
    template <class T>
    T* get(long long n) {
        const size_t b = sizeof(T) * (size_t)std::max<long long>(n, 1);
        ptrs.push_back(dmalloc(b));
        bytes += (long long)b;
        return (T*)ptrs.back();
    }
    ~Arena() {
        for (void* p : ptrs) dfree(p);
    }
};

int bit_width_of(long long n) {   // bits of n - 1, at least 1
    int b = 1;
    while ((1LL << b) < n) ++b;
    return b;
}

template <class K>
void pair_stage(long long nE, long long nR, bool distinct, const char* what, int long_pairs, int long_row,
                long long reserve_bytes, long long max_bytes, hipStream_t s, Arena& A, const long long* poff,
                const int* off, const int* iq, const int* ir, int cb, long long np, SchurPatternDev* out, bool* built) {
    // the footprint from the pair total, before anything of that size is allocated
    const int n = (int)np;
    hipcub::DoubleBuffer<K> dk(nullptr, nullptr);
    hipcub::DoubleBuffer<u64> dv(nullptr, nullptr);
    int* nullint = nullptr;
    size_t need_sort = 0, need_sel = 0, need_scan = 0, need_long = 0;
    if (np > 0) {
        OPT_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, need_sort, dk, dv, n, 0, 2 * cb, s));
        OPT_HIP_CHECK(hipcub::DeviceSelect::If(nullptr, need_sel, hipcub::CountingInputIterator<int>(0), nullint, nullint, n,
                                               IsHead<K>{nullptr}, s));
    }
    long long* nulll = nullptr;
    OPT_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, need_scan, nulll, nulll, (int)(nR + 1), s));
    // (the long lists' selects run over at most np + nR blocks / nR rows: sized for the larger)
    OPT_HIP_CHECK(hipcub::DeviceSelect::If(nullptr, need_long, hipcub::CountingInputIterator<int>(0), nullint, nullint,
                                           (int)std::min<long long>(np + nR, kMaxInt), IsLong{nullptr, 0}, s));
    const size_t need = std::max({need_sort, need_sel, need_scan, need_long, (size_t)1});
    const long long pair_bytes = (long long)(2 * sizeof(K) + sizeof(u64)) * std::max(np, 1LL);
    const long long row_bytes = (long long)(4 + 4 + 1 + 8) * (nR + 1) + 4 + 32 + 4;
    const long long transient = A.bytes + pair_bytes + row_bytes + (long long)need;
    // what stays: the pairs and, with at most np + nR blocks, the pattern's other arrays
    const long long pattern = 8 * std::max(np, 1LL) + 4 * (nR + 1) + 12 * (std::min(np + nR, kMaxInt) + 1);
    out->transient_bytes = transient;
    size_t free_b = 0, total_b = 0;
    OPT_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    if ((max_bytes >= 0 && transient > max_bytes) ||
        transient - A.bytes > (long long)free_b - pattern - std::max(reserve_bytes, 0LL)) {
        *built = false;
        return;
    }
    K* kA = A.get<K>(np);
    K* kB2 = A.get<K>(np);
    u64* vA = (u64*)dmalloc(sizeof(u64) * (size_t)std::max(np, 1LL));   // one of the two becomes the pairs
    u64* vB = (u64*)dmalloc(sizeof(u64) * (size_t)std::max(np, 1LL));
    int* first = A.get<int>(nR + 1);
    int* lt = A.get<int>(nR + 1);
    unsigned char* hasDiag = A.get<unsigned char>(nR + 1);
    long long* rp64 = A.get<long long>(nR + 1);
    int* nu_d = A.get<int>(1);
    u64* counts_d = A.get<u64>(4);
    int* nsel_d = A.get<int>(1);
    void* tmp = A.get<char>((long long)need);
    out->rowPtr = (int*)dmalloc(sizeof(int) * (size_t)(nR + 1));
    OPT_HIP_CHECK(hipMemsetAsync(nu_d, 0, sizeof(int), s));
    OPT_HIP_CHECK(hipMemsetAsync(counts_d, 0, sizeof(u64) * 4, s));
    const K* skey = kA;
    u64* spairs = vA;
    int* ustart = (int*)kB2;
    if (np > 0) {
        hipLaunchKernelGGL((sp_enumerate<K>), dim3(grid_for(np)), dim3(kB), 0, s, poff, off, iq, ir, nE, np, cb,
                           distinct ? 1 : 0, kA, vA);
        OPT_HIP_CHECK(hipGetLastError());
        dk = hipcub::DoubleBuffer<K>(kA, kB2);
        dv = hipcub::DoubleBuffer<u64>(vA, vB);
        size_t nb = need;
        OPT_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp, nb, dk, dv, n, 0, 2 * cb, s));
        skey = dk.Current();
        spairs = dv.Current();
        ustart = (int*)dk.Alternate();   // the other key buffer is free: n ints fit in n keys
        nb = need;
        OPT_HIP_CHECK(hipcub::DeviceSelect::If(tmp, nb, hipcub::CountingInputIterator<int>(0), ustart, nu_d, n,
                                               IsHead<K>{skey}, s));
    }
    out->pairs = (int*)spairs;
    // (hipFree waits for the device: the enumeration's writes into vA / vB are done by then)
    u64* spare = spairs == vA ? vB : vA;
    hipLaunchKernelGGL((sp_rows<K>), dim3(grid_for(nR + 1)), dim3(kB), 0, s, skey, (const int*)ustart, (const int*)nu_d,
                       nR, cb, first, lt, hasDiag);
    OPT_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(sp_row_counts, dim3(grid_for(nR + 1)), dim3(kB), 0, s, (const int*)first,
                       (const unsigned char*)hasDiag, nR, rp64);
    OPT_HIP_CHECK(hipGetLastError());
    size_t nb = need;
    OPT_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, nb, rp64, rp64, (int)(nR + 1), s));
    hipLaunchKernelGGL(sp_counts, dim3(grid_for(std::max(nR + 1, np))), dim3(kB), 0, s, (const long long*)rp64, nR,
                       (const int*)ustart, (const int*)nu_d, np, long_pairs, long_row, out->rowPtr, counts_d);
    OPT_HIP_CHECK(hipGetLastError());
    u64 counts[4];
    OPT_HIP_CHECK(hipMemcpyAsync(counts, counts_d, sizeof(counts), hipMemcpyDeviceToHost, s));   // read-back 2
    OPT_HIP_CHECK(hipStreamSynchronize(s));
    dfree(spare);
    const long long nnzb = (long long)counts[1];
    if (nnzb > kMaxInt)
        throw std::length_error(std::string(what) + ": more than 2^31 - 1 blocks (" + std::to_string(np) + " instance pairs)");
    out->n_blocks = nnzb;
    out->n_long = (int)counts[2];
    out->n_longrow = (int)counts[3];
    out->colInd = (int*)dmalloc(sizeof(int) * (size_t)std::max(nnzb, 1LL));
    out->blkRow = (int*)dmalloc(sizeof(int) * (size_t)std::max(nnzb, 1LL));
    out->pairPtr = (int*)dmalloc(sizeof(int) * (size_t)(nnzb + 1));
    out->longBlk = (int*)dmalloc(sizeof(int) * (size_t)std::max(out->n_long, 1));
    out->longRow = (int*)dmalloc(sizeof(int) * (size_t)std::max(out->n_longrow, 1));
    if (counts[0] > 0) {
        hipLaunchKernelGGL((sp_fill_blocks<K>), dim3(grid_for((long long)counts[0])), dim3(kB), 0, s, skey,
                           (const int*)ustart, (const int*)nu_d, cb, (const int*)out->rowPtr, (const int*)first,
                           (const unsigned char*)hasDiag, out->colInd, out->blkRow, out->pairPtr);
        OPT_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(sp_fill_diag, dim3(grid_for(nR + 1)), dim3(kB), 0, s, (const int*)ustart, (const int*)nu_d, np, nR,
                       (const int*)out->rowPtr, (const int*)first, (const int*)lt, (const unsigned char*)hasDiag,
                       out->colInd, out->blkRow, out->pairPtr);
    OPT_HIP_CHECK(hipGetLastError());
    if (out->n_long > 0) {
        nb = need;
        OPT_HIP_CHECK(hipcub::DeviceSelect::If(tmp, nb, hipcub::CountingInputIterator<int>(0), out->longBlk, nsel_d,
                                               (int)nnzb, IsLong{out->pairPtr, long_pairs}, s));
    }
    if (out->n_longrow > 0) {
        nb = need;
        OPT_HIP_CHECK(hipcub::DeviceSelect::If(tmp, nb, hipcub::CountingInputIterator<int>(0), out->longRow, nsel_d,
                                               (int)nR, IsLong{out->rowPtr, long_row}, s));
    }
    OPT_HIP_CHECK(hipStreamSynchronize(s));
    *built = true;
}

}  // namespace

void SchurPatternDev::release() {
    for (int** q : {&rowPtr, &colInd, &blkRow, &pairPtr, &pairs, &longBlk, &longRow}) {
        dfree(*q);
        *q = nullptr;
    }
}

bool schur_pattern_build_dev(long long nE, long long nR, const std::vector<SchurListDev>& lists, bool distinct,
                             const char* what, int long_pairs, int long_row, long long reserve_bytes,
                             long long max_bytes, hipStream_t s, SchurPatternDev* out) {
    *out = SchurPatternDev();
    long long nq = 0;
    for (auto& l : lists) {
        out->base.push_back(nq);
        nq += l.n;
    }
    out->n_instances = nq;
    if (nq > kMaxInt || nE > kMaxInt || nR > kMaxInt) return false;
    Arena A;
    const int ebits = bit_width_of(nE);
    // instances: the lists in their own order, then [vertex, list, position]
    int* K = A.get<int>(nq);
    int* V = A.get<int>(nq);
    int* R = A.get<int>(nq);
    int* Ks = A.get<int>(nq);
    int* iq = A.get<int>(nq);
    int* ir = A.get<int>(nq);
    int* off = A.get<int>(nE + 1);
    long long* poff = A.get<long long>(nE + 1);
    size_t need = 0, need2 = 0;
    if (nq > 0) OPT_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, need, K, Ks, V, iq, (int)nq, 0, ebits, s));
    OPT_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, need2, poff, poff, (int)(nE + 1), s));
    need = std::max({need, need2, (size_t)1});
    for (auto& l : lists)
        if (l.ev && !l.order && l.n > 0) {
            size_t nl = 0;
            OPT_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, nl, K, Ks, V, iq, (int)l.n, 0, ebits, s));
            need = std::max(need, nl);
        }
    void* tmp = A.get<char>((long long)need);
    for (size_t li = 0; li < lists.size(); ++li) {
        const SchurListDev& l = lists[li];
        if (l.n == 0) continue;
        const int* order = l.order;
        if (l.ev && !order) {   // the list's own stable sort by eliminated vertex
            int* ids = A.get<int>(l.n);
            int* ord = A.get<int>(l.n);
            hipLaunchKernelGGL(sp_iota, dim3(grid_for(l.n)), dim3(kB), 0, s, ids, l.n);
            OPT_HIP_CHECK(hipGetLastError());
            size_t nb = need;
            // (Ks is free until the global sort: the sorted keys of this list land there)
            OPT_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp, nb, l.ev, Ks, (const int*)ids, ord, (int)l.n, 0, ebits, s));
            order = ord;
        }
        hipLaunchKernelGGL(sp_gather, dim3(grid_for(l.n)), dim3(kB), 0, s, l.ev, l.rv, order, l.n, l.ebase,
                           out->base[li], K, V, R);
        OPT_HIP_CHECK(hipGetLastError());
    }
    if (nq > 0) {
        size_t nb = need;
        OPT_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp, nb, (const int*)K, Ks, (const int*)V, iq, (int)nq, 0, ebits, s));
        hipLaunchKernelGGL(sp_gather_ir, dim3(grid_for(nq)), dim3(kB), 0, s, (const int*)R, (const int*)iq, nq, ir);
        OPT_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(sp_offsets, dim3(grid_for(nE + 1)), dim3(kB), 0, s, (const int*)Ks, (int)nq, nE, distinct ? 1 : 0,
                       off, poff);
    OPT_HIP_CHECK(hipGetLastError());
    size_t nb = need;
    OPT_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, nb, poff, poff, (int)(nE + 1), s));
    long long np = 0;
    OPT_HIP_CHECK(hipMemcpyAsync(&np, poff + nE, sizeof(long long), hipMemcpyDeviceToHost, s));   // read-back 1
    OPT_HIP_CHECK(hipStreamSynchronize(s));
    if (np > kMaxInt)
        throw std::length_error(std::string(what) + ": " + std::to_string(np) + " instance pairs over " +
                                std::to_string(nq) + " edge instances (at most 2^31 - 1 of each)");
    out->n_pairs = np;
    const int cb = bit_width_of(nR);
    bool built = false;
    try {
        if (2 * cb <= 32)
            pair_stage<unsigned>(nE, nR, distinct, what, long_pairs, long_row, reserve_bytes, max_bytes, s, A, poff, off, iq,
                                 ir, cb, np, out, &built);
        else
            pair_stage<u64>(nE, nR, distinct, what, long_pairs, long_row, reserve_bytes, max_bytes, s, A, poff, off, iq, ir,
                            cb, np, out, &built);
    } catch (...) {
        out->release();
        throw;
    }
    if (!built) out->release();
    return built;
}

void schur_pattern_build_dev_host(long long nE, long long nR, const std::vector<SchurList>& lists, bool distinct,
                                  const char* what, SchurPattern* P) {
    Arena A;
    std::vector<SchurListDev> dl;
    hipStream_t s = nullptr;
    for (auto& l : lists) {
        int* rv = A.get<int>(l.n);
        int* ev = nullptr;
        if (l.n > 0) OPT_HIP_CHECK(hipMemcpyAsync(rv, l.rv, sizeof(int) * l.n, hipMemcpyHostToDevice, s));
        if (!distinct) {
            ev = A.get<int>(l.n);
            if (l.n > 0) OPT_HIP_CHECK(hipMemcpyAsync(ev, l.ev, sizeof(int) * l.n, hipMemcpyHostToDevice, s));
        }
        dl.push_back({ev, rv, nullptr, l.n, distinct && l.n > 0 ? (long long)l.ev[0] : 0LL});
    }
    OPT_HIP_CHECK(hipStreamSynchronize(s));
    SchurPatternDev D;
    if (!schur_pattern_build_dev(nE, nR, dl, distinct, what, 1 << 30, 0, 0, -1, s, &D)) {
        schur_pattern_build(nE, nR, lists, P, distinct, what);   // too large for the device: the host's answer or refusal
        return;
    }
    *P = SchurPattern();
    P->n_instances = D.n_instances;
    for (size_t l = 0; l < lists.size(); ++l) P->base.push_back(D.base[l]);
    auto down = [&](std::vector<int>& v, const int* d, long long n) {
        v.resize((size_t)n);
        if (n > 0) OPT_HIP_CHECK(hipMemcpy(v.data(), d, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
    };
    down(P->rowPtr, D.rowPtr, nR + 1);
    down(P->colInd, D.colInd, D.n_blocks);
    down(P->blkRow, D.blkRow, D.n_blocks);
    down(P->pairPtr, D.pairPtr, D.n_blocks + 1);
    down(P->pairs, D.pairs, 2 * D.n_pairs);
    D.release();
}

}  // namespace optamd
