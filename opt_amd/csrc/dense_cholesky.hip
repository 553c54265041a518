// dense_cholesky.hip — the kernels and launch chains of dense_cholesky.h.
#include "dense_cholesky.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <limits>
#include <utility>
#include <vector>

#include "common.h"

namespace optamd {

void* dmalloc(size_t bytes);
void dfree(void* p);

namespace {

constexpr int NB = kDenseNB;
constexpr int kTile = NB * NB;
constexpr int kKC = 32;   // columns of both operands staged per LDS pass of a tile product

template <typename T> struct Eps;
template <> struct Eps<float> { static constexpr float v = FLT_EPSILON; };
template <> struct Eps<double> { static constexpr double v = DBL_EPSILON; };

// One 16 x 16 x 4 MFMA. A and B operands have the same lane map in both precisions (lane l holds
// A[l & 15][l >> 4] and B[l >> 4][l & 15]); the accumulator's column is l & 15 in both, but its
// row is 4 (l >> 4) + reg in f32 and (l >> 4) + 4 reg in f64.
template <typename T> struct Mfma;
template <> struct Mfma<float> {
    typedef float Acc __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ Acc mma(float a, float b, Acc c) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ int row(int lane, int reg) { return (lane >> 4) * 4 + reg; }
};
template <> struct Mfma<double> {
    typedef double Acc __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ Acc mma(double a, double b, Acc c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ int row(int lane, int reg) { return (lane >> 4) + 4 * reg; }
};

// A wave's part of a 64 x 64 tile product as MFMA accumulators: wave w owns rows 16 w .. 16 w + 15
// in four 16 x 16 accumulators, one per 16 columns. (The f32 32 x 32 x 2 form, one 32 x 32
// quadrant per wave, measured the same: DESIGN 3.6, Direct solver.)
template <typename T>
struct Frag16 {
    static constexpr int kStep = 4;
    typename Mfma<T>::Acc acc[4];
    __device__ __forceinline__ static int at(int n, int r) {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        return (w * 16 + Mfma<T>::row(lane, r)) * NB + n * 16 + (lane & 15);
    }
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[n][r] = (T)0;
    }
    __device__ __forceinline__ void load(const T* C) {
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[n][r] = C[at(n, r)];
    }
    __device__ __forceinline__ void store(T* C) const {
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) C[at(n, r)] = acc[n][r];
    }
    template <bool kNegate>
    __device__ __forceinline__ void step(T (*As)[kKC + 1], T (*Bs)[kKC + 1], int kk) {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        T a = As[w * 16 + (lane & 15)][kk + (lane >> 4)];
        if (kNegate) a = -a;
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[n] = Mfma<T>::mma(a, Bs[n * 16 + (lane & 15)][kk + (lane >> 4)], acc[n]);
    }
};
// f += sign * A B^T for two row-major NB x NB tiles, by the 4 waves of a 256-thread workgroup.
// Both operands pass through LDS kKC columns at a time; the sum over k runs ascending. A may
// alias the tile the caller stores the product to: its last read is before this returns.
template <typename T, bool kNegate, class Frag>
__device__ __forceinline__ void tile_abt(const T* A, const T* __restrict__ B, T (*As)[kKC + 1], T (*Bs)[kKC + 1], Frag& f) {
    const int tid = threadIdx.x;
    for (int k0 = 0; k0 < NB; k0 += kKC) {
        __syncthreads();   // the previous pass's reads
        for (int e = tid; e < NB * kKC; e += 256) {
            const int r = e / kKC, c = e % kKC;
            As[r][c] = A[r * NB + k0 + c];
            Bs[r][c] = B[r * NB + k0 + c];
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kKC; kk += Frag::kStep) f.template step<kNegate>(As, Bs, kk);
    }
}

__global__ void dense_reset_kernel(DenseStatus* st) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        st->fail = -1;
        st->pad = 0;
        st->ratio = INFINITY;
    }
}

// tile number t of the packed lower triangle -> (I, J)
__device__ __forceinline__ void tile_of(long long t, int* I, int* J) {
    long long i = (long long)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (i * (i + 1) / 2 > t) --i;
    while ((i + 1) * (i + 2) / 2 <= t) ++i;
    *I = (int)i;
    *J = (int)(t - i * (i + 1) / 2);
}

// One workgroup per tile of the lower triangle: the tile from the row-major matrix, identity in
// the padding; the diagonal tiles' workgroups also write the original diagonal and the padded
// right-hand side.
template <typename T>
__global__ __launch_bounds__(256) void dense_fill_kernel(long long n, const T* __restrict__ A, const T* __restrict__ b,
                                                         T* __restrict__ tiles, T* __restrict__ diag0, T* __restrict__ rhs) {
    int I, J;
    tile_of(blockIdx.x, &I, &J);
    T* out = tiles + dense_tile(I, J);
    for (int e = threadIdx.x; e < kTile; e += 256) {
        const long long gi = (long long)I * NB + (e >> 6), gj = (long long)J * NB + (e & 63);
        out[e] = gi < n && gj < n ? A[gi * n + gj] : (gi == gj ? (T)1 : (T)0);
    }
    if (I == J && threadIdx.x < NB) {
        const long long gi = (long long)I * NB + threadIdx.x;
        diag0[gi] = gi < n ? A[gi * n + gi] : (T)1;
        rhs[gi] = gi < n ? b[gi] : (T)0;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void dense_extract_kernel(long long n, const T* __restrict__ tiles, T* __restrict__ L) {
    int I, J;
    tile_of(blockIdx.x, &I, &J);
    const T* in = tiles + dense_tile(I, J);
    for (int e = threadIdx.x; e < kTile; e += 256) {
        const long long gi = (long long)I * NB + (e >> 6), gj = (long long)J * NB + (e & 63);
        if (gi < n && gj <= gi) L[gi * n + gj] = in[e];
    }
}

// Tile (k, k) = L_kk L_kk^T in LDS by one workgroup; L_kk (upper triangle zero) back in place and
// L_kk^-1 to inv. The inverse's strict lower triangle is built transposed in the LDS tile's upper
// triangle: thread c owns column c of it and reads only L and its own column.
template <typename T>
__global__ __launch_bounds__(256) void dense_potrf_kernel(T* __restrict__ tile, T* __restrict__ inv,
                                                          const T* __restrict__ diag0, long long row0, DenseStatus* st) {
    if (st->fail >= 0) return;
    __shared__ T a[NB][NB + 1];
    const int tid = threadIdx.x;
    for (int e = tid; e < kTile; e += 256) {
        const int r = e >> 6, c = e & 63;
        a[r][c] = c <= r ? tile[e] : (T)0;
    }
    double ratio = INFINITY;
    for (int j = 0; j < NB; ++j) {
        __syncthreads();
        const T d = a[j][j], d0 = diag0[j];   // the same two values in every thread
        if (!(d > Eps<T>::v * d0) || !(d > (T)0)) {   // (NaN fails both)
            if (tid == 0) st->fail = (int)(row0 + j);
            return;
        }
        ratio = fmin(ratio, (double)d / (double)d0);
        const T l = sqrt(d);
        __syncthreads();   // every thread has read the pivot
        if (tid == j) a[j][j] = l;
        else if (tid > j && tid < NB) a[tid][j] = a[tid][j] / l;
        __syncthreads();
        for (int e = tid; e < kTile; e += 256) {
            const int i = e >> 6, c = e & 63;
            if (c > j && c <= i) a[i][c] -= a[i][j] * a[c][j];
        }
    }
    __syncthreads();
    if (tid < NB) {
        const int c = tid;
        const T xc = (T)1 / a[c][c];
        for (int i = c + 1; i < NB; ++i) {
            T s = a[i][c] * xc;
            for (int m = c + 1; m < i; ++m) s += a[i][m] * a[c][m];
            a[c][i] = -s / a[i][i];
        }
    }
    __syncthreads();
    for (int e = tid; e < kTile; e += 256) {
        const int r = e >> 6, c = e & 63;
        tile[e] = c <= r ? a[r][c] : (T)0;
        inv[e] = c < r ? a[c][r] : (c == r ? (T)1 / a[r][r] : (T)0);
    }
    if (tid == 0 && ratio < st->ratio) st->ratio = ratio;
}

// A_Ik <- A_Ik L_kk^-T for I = k + 1 + blockIdx.x
template <typename T>
__global__ __launch_bounds__(256) void dense_panel_kernel(T* tiles, const T* __restrict__ invk, int k, const DenseStatus* st) {
    if (st->fail >= 0) return;
    __shared__ T As[NB][kKC + 1], Bs[NB][kKC + 1];
    T* A = tiles + dense_tile(k + 1 + (int)blockIdx.x, k);
    Frag16<T> f;
    f.zero();
    tile_abt<T, false>(A, invk, As, Bs, f);
    f.store(A);
}

// A_IJ -= A_Ik A_Jk^T for I = k + 1 + blockIdx.y, J = k + 1 + blockIdx.x, J <= I: the accumulator
// starts as A_IJ and takes the products of the negated left operand.
template <typename T>
__global__ __launch_bounds__(256) void dense_update_kernel(T* tiles, int k, const DenseStatus* st) {
    if (blockIdx.x > blockIdx.y) return;
    if (st->fail >= 0) return;
    __shared__ T As[NB][kKC + 1], Bs[NB][kKC + 1];
    const int I = k + 1 + (int)blockIdx.y, J = k + 1 + (int)blockIdx.x;
    T* C = tiles + dense_tile(I, J);
    Frag16<T> f;
    f.load(C);
    tile_abt<T, true>(tiles + dense_tile(I, k), tiles + dense_tile(J, k), As, Bs, f);
    f.store(C);
}

// Forward launch k: segment I = k + blockIdx.x takes b_I -= L_{I,k-1} y_{k-1} (k > 0); the
// workgroup of I = k then forms y_k = L_kk^-1 b_k. 64 threads, one per row.
template <typename T>
__global__ __launch_bounds__(NB) void dense_forward_kernel(const T* __restrict__ tiles, const T* __restrict__ inv, T* b,
                                                           int k, const DenseStatus* st) {
    if (st->fail >= 0) return;
    __shared__ T y[NB];
    __shared__ T Ls[NB][NB + 1];   // the tile, read with whole rows per instruction (lane t then walks row t)
    const int t = threadIdx.x, I = k + (int)blockIdx.x;
    T bi = b[(long long)I * NB + t];
    if (k > 0) {
        y[t] = b[(long long)(k - 1) * NB + t];
        const T* L = tiles + dense_tile(I, k - 1);
        for (int e = t; e < kTile; e += NB) Ls[e >> 6][e & 63] = L[e];
        __syncthreads();
        T s = 0;
        for (int c = 0; c < NB; ++c) s += Ls[t][c] * y[c];
        bi -= s;
    }
    if (I == k) {
        __syncthreads();
        y[t] = bi;
        const T* V = inv + (long long)k * kTile;
        for (int e = t; e < kTile; e += NB) Ls[e >> 6][e & 63] = V[e];
        __syncthreads();
        T s = 0;
        for (int c = 0; c <= t; ++c) s += Ls[t][c] * y[c];
        bi = s;
    }
    b[(long long)I * NB + t] = bi;
}

// Backward launch j (from the last panel down): segment K = blockIdx.x <= j takes
// b_K -= L_{j+1,K}^T x_{j+1} (j below the last); the workgroup of K = j then forms
// x_j = L_jj^-T b_j.
template <typename T>
__global__ __launch_bounds__(NB) void dense_backward_kernel(const T* __restrict__ tiles, const T* __restrict__ inv, T* b,
                                                            int j, int nt, const DenseStatus* st) {
    if (st->fail >= 0) return;
    __shared__ T y[NB];
    const int t = threadIdx.x, K = (int)blockIdx.x;
    T bi = b[(long long)K * NB + t];
    if (j < nt - 1) {
        y[t] = b[(long long)(j + 1) * NB + t];
        __syncthreads();
        const T* L = tiles + dense_tile(j + 1, K) + t;
        T s = 0;
        for (int r = 0; r < NB; ++r) s += L[r * NB] * y[r];
        bi -= s;
    }
    if (K == j) {
        __syncthreads();
        y[t] = bi;
        __syncthreads();
        const T* V = inv + (long long)j * kTile + t;
        T s = 0;
        for (int r = t; r < NB; ++r) s += V[r * NB] * y[r];
        bi = s;
    }
    b[(long long)K * NB + t] = bi;
}

// ---- blocks of A^-1 (DenseSelection in dense_cholesky.h) ----
// X(R, I) of the transposed right-hand sides
__device__ __forceinline__ long long cov_tile(long long R, long long I, int nt) { return (R * nt + I) * (long long)kTile; }

// Seed, one workgroup per tile (I, R) with I >= start(R): zero, then the one of each selected
// unknown of the tile-row that falls into panel I (written by the thread that zeroed the row's
// entries or another: the barrier between orders them).
template <typename T>
__global__ __launch_bounds__(256) void dense_cov_seed_kernel(T* __restrict__ X, const int* __restrict__ unknown,
                                                             const int* __restrict__ start, int nt, const DenseStatus* st) {
    if (st->fail >= 0) return;
    const int I = (int)blockIdx.x, R = (int)blockIdx.y;
    if (I < start[R]) return;
    T* x = X + cov_tile(R, I, nt);
    for (int e = threadIdx.x; e < kTile; e += 256) x[e] = (T)0;
    __syncthreads();
    if (threadIdx.x < NB) {
        const int g = unknown[R * NB + (int)threadIdx.x];
        if (g >= 0 && (g >> 6) == I) x[(int)threadIdx.x * NB + (g & 63)] = (T)1;
    }
}

// Diagonal step of panel k: X(R, k) <- X(R, k) L_kk^-T for the live tile-row R = blockIdx.x
template <typename T>
__global__ __launch_bounds__(256) void dense_cov_diag_kernel(T* X, const T* __restrict__ invk, int k, int nt, const DenseStatus* st) {
    if (st->fail >= 0) return;
    __shared__ T As[NB][kKC + 1], Bs[NB][kKC + 1];
    T* A = X + cov_tile(blockIdx.x, k, nt);
    Frag16<T> f;
    f.zero();
    tile_abt<T, false>(A, invk, As, Bs, f);
    f.store(A);
}

// Trailing step of panel k: X(R, I) -= X(R, k) L(I, k)^T for I = k + 1 + blockIdx.x, R = blockIdx.y
template <typename T>
__global__ __launch_bounds__(256) void dense_cov_trail_kernel(T* X, const T* __restrict__ tiles, int k, int nt, const DenseStatus* st) {
    if (st->fail >= 0) return;
    __shared__ T As[NB][kKC + 1], Bs[NB][kKC + 1];
    const int I = k + 1 + (int)blockIdx.x, R = (int)blockIdx.y;
    T* C = X + cov_tile(R, I, nt);
    Frag16<T> f;
    f.load(C);
    tile_abt<T, true>(X + cov_tile(R, k, nt), tiles + dense_tile(I, k), As, Bs, f);
    f.store(C);
}

// Gram tile p = (R, R'): sum over I of X(R, I) X(R', I)^T, I ascending from the later start
template <typename T>
__global__ __launch_bounds__(256) void dense_cov_gram_kernel(const T* __restrict__ X, const int* __restrict__ start,
                                                             const int* __restrict__ gramR, const int* __restrict__ gramC,
                                                             T* __restrict__ G, int nt, const DenseStatus* st) {
    if (st->fail >= 0) return;
    __shared__ T As[NB][kKC + 1], Bs[NB][kKC + 1];
    const int R = gramR[blockIdx.x], Rc = gramC[blockIdx.x];
    Frag16<T> f;
    f.zero();
    for (int I = max(start[R], start[Rc]); I < nt; ++I)
        tile_abt<T, false>(X + cov_tile(R, I, nt), X + cov_tile(Rc, I, nt), As, Bs, f);
    f.store(G + (long long)blockIdx.x * kTile);
}

// Requested block q out of its Gram tile, one thread per entry; zeros where the mask holds a 0
// for either element.
template <typename T>
__global__ __launch_bounds__(256) void dense_cov_gather_kernel(const T* __restrict__ G, const int* __restrict__ blk, int C,
                                                               long long nPairs, const T* __restrict__ mask,
                                                               T* __restrict__ out, const DenseStatus* st) {
    if (st->fail >= 0) return;
    const long long CC = (long long)C * C, total = nPairs * CC;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long q = e / CC;
        const int ij = (int)(e - q * CC), i = ij / C, j = ij - i * C;
        const int* b = blk + q * 5;
        const bool on = !mask || (mask[(long long)b[3] * C] != (T)0 && mask[(long long)b[4] * C] != (T)0);
        out[e] = on ? G[(long long)b[0] * kTile + (b[1] + i) * NB + b[2] + j] : (T)0;
    }
}

size_t cov_align(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

bool DenseSelection::build(long long n_, int C_, long long nPairs_, const int* rowElem, const int* colElem) {
    // (n: the grids of the seed and the trailing step stay below 65536 a side)
    if (n_ < 1 || n_ > 2000000 || C_ < 1 || C_ > NB || n_ % C_ != 0 || nPairs_ < 0 || (nPairs_ > 0 && (!rowElem || !colElem))) return false;
    const long long ne = n_ / C_;
    for (long long q = 0; q < nPairs_; ++q)
        if (rowElem[q] < 0 || rowElem[q] >= ne || colElem[q] < 0 || colElem[q] >= ne) return false;
    n = n_, C = C_, nPairs = nPairs_, nt = dense_tiles_per_side(n_);
    std::vector<char> sel((size_t)ne, 0);
    for (long long q = 0; q < nPairs; ++q) sel[rowElem[q]] = sel[colElem[q]] = 1;
    std::vector<int> slot((size_t)ne, -1);   // element -> its place in the sorted selection
    const int per = NB / C;
    long long m = 0;
    unknown.clear();
    start.clear();
    for (long long e = 0; e < ne; ++e) {
        if (!sel[e]) continue;
        if (m % per == 0) {
            unknown.insert(unknown.end(), NB, -1);
            start.push_back((int)(e * C / NB));
        }
        for (int i = 0; i < C; ++i) unknown[(m / per) * NB + (m % per) * C + i] = (int)(e * C + i);
        slot[e] = (int)m++;
    }
    tile_rows = (long long)start.size();
    x_tiles = tile_rows * nt;
    live.assign((size_t)nt, 0);
    for (long long k = 0, R = 0; k < nt; ++k) {
        while (R < tile_rows && start[R] <= k) ++R;
        live[k] = (int)R;
    }
    gramR.clear();
    gramC.clear();
    blk.assign((size_t)nPairs * 5, 0);
    std::vector<std::pair<long long, long long>> order((size_t)nPairs);   // (tile-row pair, request), to number the distinct pairs
    for (long long q = 0; q < nPairs; ++q)
        order[q] = {(long long)(slot[rowElem[q]] / per) * tile_rows + slot[colElem[q]] / per, q};
    std::sort(order.begin(), order.end());
    for (long long o = 0; o < nPairs; ++o) {
        const long long q = order[o].second;
        if (o == 0 || order[o].first != order[o - 1].first) {
            gramR.push_back((int)(order[o].first / tile_rows));
            gramC.push_back((int)(order[o].first % tile_rows));
        }
        int* b = &blk[q * 5];
        b[0] = (int)gramR.size() - 1;
        b[1] = (slot[rowElem[q]] % per) * C;
        b[2] = (slot[colElem[q]] % per) * C;
        b[3] = rowElem[q];
        b[4] = colElem[q];
    }
    gram_tiles = (long long)gramR.size();
    return true;
}

double DenseSelection::forward_flops() const {
    double products = 0;
    for (long long R = 0; R < tile_rows; ++R) {
        const double m = (double)(nt - start[R]);
        products += m * (m + 1) / 2;   // one diagonal and nt - k - 1 trailing products per live panel
    }
    return products * 2.0 * NB * NB * NB;
}

size_t dense_cov_bytes(const DenseSelection& sel, size_t elem) {
    return cov_align((size_t)sel.x_tiles * kTile * elem) + cov_align((size_t)sel.gram_tiles * kTile * elem) +
           cov_align(sizeof(int) * (sel.unknown.size() + sel.start.size() + sel.gramR.size() + sel.gramC.size() + sel.blk.size() + 1));
}

size_t dense_bytes(long long n, size_t elem) {
    const long long nt = dense_tiles_per_side(n);
    return ((size_t)dense_tile_count(n) + (size_t)nt) * kTile * elem + 2 * (size_t)nt * NB * elem + sizeof(DenseStatus);
}

template <typename T>
void DenseFactor<T>::release() {
    for (T** q : {&tiles_, &inv_, &diag0_, &rhs_}) {
        dfree(*q);
        *q = nullptr;
    }
    dfree(st_);
    st_ = nullptr;
    dfree(ws_);
    ws_ = nullptr;
    ws_bytes_ = 0;
    n_ = nt_ = 0;
}

template <typename T>
void DenseFactor<T>::resize(long long n) {
    if (n == n_ && tiles_) return;
    release();
    n_ = n;
    nt_ = dense_tiles_per_side(n);
    tiles_ = (T*)dmalloc(sizeof(T) * (size_t)dense_tile_count(n) * kTile);
    inv_ = (T*)dmalloc(sizeof(T) * (size_t)nt_ * kTile);
    diag0_ = (T*)dmalloc(sizeof(T) * (size_t)nt_ * NB);
    rhs_ = (T*)dmalloc(sizeof(T) * (size_t)nt_ * NB);
    st_ = (DenseStatus*)dmalloc(sizeof(DenseStatus));
}

template <typename T>
void DenseFactor<T>::reset(hipStream_t s) {
    dense_reset_kernel<<<1, 64, 0, s>>>(st_);
}

template <typename T>
void DenseFactor<T>::fill_from_dense(const T* A, const T* b, hipStream_t s) {
    reset(s);
    dense_fill_kernel<T><<<(unsigned)dense_tile_count(n_), 256, 0, s>>>(n_, A, b, tiles_, diag0_, rhs_);
    OPT_HIP_CHECK(hipGetLastError());
}

template <typename T>
void DenseFactor<T>::factor(hipStream_t s) {
    const int nt = (int)nt_;
    for (int k = 0; k < nt; ++k) {
        dense_potrf_kernel<T><<<1, 256, 0, s>>>(tiles_ + dense_tile(k, k), inv_ + (long long)k * kTile,
                                               diag0_ + (long long)k * NB, (long long)k * NB, st_);
        const int m = nt - k - 1;
        if (m > 0) {
            dense_panel_kernel<T><<<m, 256, 0, s>>>(tiles_, inv_ + (long long)k * kTile, k, st_);
            dense_update_kernel<T><<<dim3(m, m), 256, 0, s>>>(tiles_, k, st_);
        }
    }
    OPT_HIP_CHECK(hipGetLastError());
}

template <typename T>
void DenseFactor<T>::solve(hipStream_t s) {
    const int nt = (int)nt_;
    for (int k = 0; k < nt; ++k) dense_forward_kernel<T><<<nt - k, NB, 0, s>>>(tiles_, inv_, rhs_, k, st_);
    for (int j = nt - 1; j >= 0; --j) dense_backward_kernel<T><<<j + 1, NB, 0, s>>>(tiles_, inv_, rhs_, j, nt, st_);
    OPT_HIP_CHECK(hipGetLastError());
}

template <typename T>
int DenseFactor<T>::status(hipStream_t s, double* min_ratio) {
    DenseStatus h;
    OPT_HIP_CHECK(hipMemcpyAsync(&h, st_, sizeof(h), hipMemcpyDeviceToHost, s));
    OPT_HIP_CHECK(hipStreamSynchronize(s));
    if (min_ratio) *min_ratio = h.ratio;
    return h.fail;
}

template <typename T>
void DenseFactor<T>::extract_lower(T* L, hipStream_t s) const {
    dense_extract_kernel<T><<<(unsigned)dense_tile_count(n_), 256, 0, s>>>(n_, tiles_, L);
    OPT_HIP_CHECK(hipGetLastError());
}

namespace {
// the parts of the covariance workspace, in the order dense_cov_bytes sums them
template <typename T>
struct CovParts {
    T *X, *G;
    int *unknown, *start, *gramR, *gramC, *blk;
    CovParts(char* ws, const DenseSelection& sel) {
        X = (T*)ws;
        G = (T*)(ws + cov_align((size_t)sel.x_tiles * kTile * sizeof(T)));
        unknown = (int*)((char*)G + cov_align((size_t)sel.gram_tiles * kTile * sizeof(T)));
        start = unknown + sel.unknown.size();
        gramR = start + sel.start.size();
        gramC = gramR + sel.gramR.size();
        blk = gramC + sel.gramC.size();
    }
};
}  // namespace

template <typename T>
void DenseFactor<T>::cov_begin(const DenseSelection& sel, hipStream_t s) {
    const size_t need = dense_cov_bytes(sel, sizeof(T));
    if (need != ws_bytes_) {
        dfree(ws_);
        ws_ = nullptr;
        ws_bytes_ = 0;
        ws_ = (char*)dmalloc(need);
        ws_bytes_ = need;
    }
    if (sel.nPairs == 0) return;
    const CovParts<T> w(ws_, sel);
    for (auto cp : {std::make_pair(w.unknown, &sel.unknown), std::make_pair(w.start, &sel.start), std::make_pair(w.gramR, &sel.gramR),
                    std::make_pair(w.gramC, &sel.gramC), std::make_pair(w.blk, &sel.blk)})
        OPT_HIP_CHECK(hipMemcpyAsync(cp.first, cp.second->data(), sizeof(int) * cp.second->size(), hipMemcpyHostToDevice, s));
    OPT_HIP_CHECK(hipStreamSynchronize(s));   // (the selection's vectors are the caller's again)
    dense_cov_seed_kernel<T><<<dim3((unsigned)nt_, (unsigned)sel.tile_rows), 256, 0, s>>>(w.X, w.unknown, w.start, (int)nt_, st_);
    OPT_HIP_CHECK(hipGetLastError());
}

template <typename T>
void DenseFactor<T>::cov_forward(const DenseSelection& sel, hipStream_t s) {
    if (sel.nPairs == 0) return;
    const CovParts<T> w(ws_, sel);
    const int nt = (int)nt_;
    for (int k = 0; k < nt; ++k) {
        const int live = sel.live[k];
        if (live == 0) continue;
        dense_cov_diag_kernel<T><<<live, 256, 0, s>>>(w.X, inv_ + (long long)k * kTile, k, nt, st_);
        if (nt - k - 1 > 0) dense_cov_trail_kernel<T><<<dim3(nt - k - 1, live), 256, 0, s>>>(w.X, tiles_, k, nt, st_);
    }
    OPT_HIP_CHECK(hipGetLastError());
}

template <typename T>
void DenseFactor<T>::cov_gram(const DenseSelection& sel, const T* mask, T* out, hipStream_t s) {
    if (sel.nPairs == 0) return;
    const CovParts<T> w(ws_, sel);
    dense_cov_gram_kernel<T><<<(unsigned)sel.gram_tiles, 256, 0, s>>>(w.X, w.start, w.gramR, w.gramC, w.G, (int)nt_, st_);
    const long long total = sel.nPairs * sel.C * sel.C;
    dense_cov_gather_kernel<T><<<(unsigned)std::min<long long>((total + 255) / 256, 1 << 16), 256, 0, s>>>(w.G, w.blk, sel.C, sel.nPairs,
                                                                                                        mask, out, st_);
    OPT_HIP_CHECK(hipGetLastError());
}

template class DenseFactor<float>;
template class DenseFactor<double>;

template <typename T>
long long dense_cholesky_host(long long n, const T* A, const T* b, T* L, T* x) {
    const size_t dense = sizeof(T) * (size_t)n * (size_t)n, vec = sizeof(T) * (size_t)n;
    size_t free_b = 0, total_b = 0;
    OPT_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    if (dense_bytes(n, sizeof(T)) + dense + vec > free_b) return -2;
    T* dA = (T*)dmalloc(dense);
    T* db = (T*)dmalloc(vec);
    OPT_HIP_CHECK(hipMemcpy(dA, A, dense, hipMemcpyHostToDevice));
    OPT_HIP_CHECK(hipMemcpy(db, b, vec, hipMemcpyHostToDevice));
    long long fail;
    {
        DenseFactor<T> F;
        F.resize(n);
        F.fill_from_dense(dA, db, nullptr);
        F.factor(nullptr);
        F.solve(nullptr);
        fail = F.status(nullptr, nullptr);
        if (fail < 0) {
            OPT_HIP_CHECK(hipMemsetAsync(dA, 0, dense, nullptr));
            F.extract_lower(dA, nullptr);
            OPT_HIP_CHECK(hipMemcpy(L, dA, dense, hipMemcpyDeviceToHost));
            OPT_HIP_CHECK(hipMemcpy(x, F.solution(), vec, hipMemcpyDeviceToHost));
        }
        OPT_HIP_CHECK(hipDeviceSynchronize());
    }
    dfree(dA);
    dfree(db);
    return fail;
}
template long long dense_cholesky_host<float>(long long, const float*, const float*, float*, float*);
template long long dense_cholesky_host<double>(long long, const double*, const double*, double*, double*);

template <typename T>
long long dense_inverse_blocks_host(long long n, const T* A, const DenseSelection& sel, T* out) {
    const size_t dense = sizeof(T) * (size_t)n * (size_t)n, vec = sizeof(T) * (size_t)n;
    const size_t blocks = sizeof(T) * (size_t)sel.nPairs * sel.C * sel.C;
    size_t free_b = 0, total_b = 0;
    OPT_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    if (dense_bytes(n, sizeof(T)) + dense_cov_bytes(sel, sizeof(T)) + dense + vec + blocks > free_b) return -2;
    T* dA = (T*)dmalloc(dense);
    T* db = (T*)dmalloc(vec);
    T* dout = (T*)dmalloc(blocks ? blocks : sizeof(T));
    OPT_HIP_CHECK(hipMemcpy(dA, A, dense, hipMemcpyHostToDevice));
    OPT_HIP_CHECK(hipMemset(db, 0, vec));
    long long fail;
    {
        DenseFactor<T> F;
        F.resize(n);
        F.fill_from_dense(dA, db, nullptr);
        F.factor(nullptr);
        fail = F.status(nullptr, nullptr);
        if (fail < 0) {
            F.covariance(sel, nullptr, dout, nullptr);
            if (blocks) OPT_HIP_CHECK(hipMemcpy(out, dout, blocks, hipMemcpyDeviceToHost));
        }
        OPT_HIP_CHECK(hipDeviceSynchronize());
    }
    dfree(dA);
    dfree(db);
    dfree(dout);
    return fail;
}
template long long dense_inverse_blocks_host<float>(long long, const float*, const DenseSelection&, float*);
template long long dense_inverse_blocks_host<double>(long long, const double*, const DenseSelection&, double*);

}  // namespace optamd
