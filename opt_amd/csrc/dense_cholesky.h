// dense_cholesky.h — a dense blocked Cholesky factorisation A = L L^T and the two triangular
// solves on the device (dense_cholesky.hip), in float and double. Nothing here depends on an
// energy: the kernels are compiled into the library, not generated.
//
// Storage: the lower triangle in kDenseNB x kDenseNB tiles; tile (I, J), I >= J, sits at
// dense_tile(I, J) and is row-major inside. n is padded to a multiple of kDenseNB with 1 on the
// padded diagonal and 0 in the padded right-hand side, so the padding solves to 0 and never
// reaches the caller.
//
// Factorisation: right-looking, three launches per panel k — potrf (one workgroup factors tile
// (k, k) in LDS, applies the pivot rule and leaves L_kk^-1 in a side buffer), panel (A_Ik <-
// A_Ik L_kk^-T, I > k) and trailing update (A_IJ -= A_Ik A_Jk^T, k < J <= I). Panel and update
// are MFMA products (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64), summed k ascending, so
// two runs agree bitwise. Solves: one launch per panel, forward then backward; every segment of
// the right-hand side has one writer per launch. The launch chain is the only ordering: no
// kernel waits for another workgroup, and there are no atomics.
//
// Pivot rule: the pivot of row i fails when it is NaN, not positive, or <= eps * a_ii with a_ii
// the entry of the matrix as filled and eps the precision's machine epsilon. The potrf kernel
// that meets it stores the row in DenseStatus::fail (a plain store by one thread of the only
// workgroup of that launch); every later kernel of the chain returns at entry when it is set.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <vector>

namespace optamd {

constexpr int kDenseNB = 64;

__host__ __device__ inline long long dense_tile(long long I, long long J) {
    return (I * (I + 1) / 2 + J) * (long long)(kDenseNB * kDenseNB);
}
inline long long dense_tiles_per_side(long long n) { return (n + kDenseNB - 1) / kDenseNB; }
inline long long dense_tile_count(long long n) {
    const long long nt = dense_tiles_per_side(n);
    return nt * (nt + 1) / 2;
}
// everything a DenseFactor<T> of dimension n allocates
size_t dense_bytes(long long n, size_t elem);

struct DenseStatus {
    int fail;       // first row whose pivot failed, -1 while none has
    int pad;
    double ratio;   // smallest pivot / original diagonal entry met so far
};

// Blocks of A^-1 from the factor (DenseFactor::covariance): A^-1 = L^-T L^-1, so the C x C block
// (s, t) is Y_s^T Y_t with Y = L^-1 E and E the identity columns of the selected unknowns. The
// right-hand sides are stored transposed, X = Y^T: one row per selected unknown, n columns, in
// 64 x 64 tiles X(R, I), tile-row R major. The distinct selected elements are sorted ascending and
// packed floor(64 / C) to a tile-row (unused rows zero), so no element straddles two tile-rows and
// every requested block lies inside one Gram tile G(R, R') = sum_I X(R, I) X(R', I)^T. X(R, I) is
// identically zero for I < start(R) = floor(first selected unknown of R / 64): those tiles are
// never written, read or multiplied. start is non-decreasing in R, so the tile-rows live at panel
// k are the prefix R < live(k).
//
// Forward chain, right-looking, two launches per panel k over the live prefix: the diagonal step
// X(R, k) <- X(R, k) L_kk^-T (the dense_panel shape) and the trailing step X(R, I) -= X(R, k)
// L(I, k)^T, I > k (the dense_update shape). Then one Gram workgroup per needed (R, R'), its sum
// over I ascending from max(start(R), start(R')), and a gather of the requested blocks. The
// selection is laid out on the host, once per call.
struct DenseSelection {
    // elements of C unknowns each, 64 % C need not be 0, 1 <= C <= 64; every index in [0, n / C).
    // false (nothing built) on a bad index, C out of range or n no multiple of C.
    bool build(long long n, int C, long long nPairs, const int* rowElem, const int* colElem);
    long long n = 0, nt = 0, nPairs = 0, tile_rows = 0, gram_tiles = 0, x_tiles = 0;
    int C = 0;
    std::vector<int> unknown;     // tile_rows x 64: the unknown of each row of X, -1 where unused
    std::vector<int> start;       // per tile-row
    std::vector<int> live;        // per panel: tile-rows with start <= k
    std::vector<int> gramR, gramC;   // per Gram tile: its two tile-rows
    std::vector<int> blk;         // per requested block: Gram tile, first row, first column, row element, column element
    // flops of the forward chain (2 * 64^3 per tile product)
    double forward_flops() const;
};
// what DenseFactor<T>::covariance allocates for a selection, beside dense_bytes
size_t dense_cov_bytes(const DenseSelection& sel, size_t elem);

template <typename T>
class DenseFactor {
public:
    DenseFactor() = default;
    DenseFactor(const DenseFactor&) = delete;
    DenseFactor& operator=(const DenseFactor&) = delete;
    ~DenseFactor() { release(); }

    // storage for dimension n (n >= 1); what an earlier size held is freed first
    void resize(long long n);
    void release();
    long long n() const { return n_; }
    long long tiles_per_side() const { return nt_; }

    // fail = -1, ratio = +inf: the first launch of every fill
    void reset(hipStream_t s);
    // tiles, original diagonal and right-hand side from a device row-major n x n matrix (both
    // triangles are read) and a device vector
    void fill_from_dense(const T* A, const T* b, hipStream_t s);
    void factor(hipStream_t s);
    // L y = b, L^T x = y in place of the padded right-hand side
    void solve(hipStream_t s);
    // one small copy and one stream sync: the failing row or -1, the smallest pivot ratio
    int status(hipStream_t s, double* min_ratio);
    // Blocks of A^-1 after factor() (DenseSelection above): out[q][C][C] on the device for request
    // q. mask (may be null): one value per unknown, 0 marks an unknown whose blocks and cross
    // blocks are returned as zeros. covariance() is the three stages in order; a plan brackets
    // them with its timer. The workspace is sized by cov_begin and freed with the factor.
    void covariance(const DenseSelection& sel, const T* mask, T* out, hipStream_t s) {
        cov_begin(sel, s);
        cov_forward(sel, s);
        cov_gram(sel, mask, out, s);
    }
    void cov_begin(const DenseSelection& sel, hipStream_t s);     // workspace, the layout uploaded, the seed
    void cov_forward(const DenseSelection& sel, hipStream_t s);
    void cov_gram(const DenseSelection& sel, const T* mask, T* out, hipStream_t s);   // Gram tiles and gather
    size_t cov_capacity() const { return ws_bytes_; }
    // the factor as a device row-major n x n matrix (lower triangle written, padding dropped)
    void extract_lower(T* L, hipStream_t s) const;

    T* tiles() { return tiles_; }
    T* diag0() { return diag0_; }
    T* rhs() { return rhs_; }
    const T* solution() const { return rhs_; }
    DenseStatus* status_dev() { return st_; }

private:
    long long n_ = 0, nt_ = 0;
    T *tiles_ = nullptr, *inv_ = nullptr, *diag0_ = nullptr, *rhs_ = nullptr;
    DenseStatus* st_ = nullptr;
    char* ws_ = nullptr;          // covariance workspace: X, the Gram tiles, the selection's index arrays
    size_t ws_bytes_ = 0;
};

// Host arrays in, host arrays out (OptAMD_DenseCholesky): fill, factor and solve on the current
// device's null stream. Returns the first failing row (L and x untouched) or -1; -2 where the
// storage does not fit the device.
template <typename T>
long long dense_cholesky_host(long long n, const T* A, const T* b, T* L, T* x);

// Host arrays in, host array out (OptAMD_DenseInverseBlocks): fill, factor and covariance() for a
// selection built by the caller. Returns the first failing row (out untouched) or -1; -2 where
// the storage does not fit the device.
template <typename T>
long long dense_inverse_blocks_host(long long n, const T* A, const DenseSelection& sel, T* out);

}  // namespace optamd
