// dense_cholesky.hip — the kernels and launch chains of dense_cholesky.h.
#include "dense_cholesky.h"

#include <cfloat>
#include <cmath>
#include <limits>

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

}  // namespace

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

}  // namespace optamd
