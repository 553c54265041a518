// gen/codegen_dense.cpp — the two layout-aware kernels of LinearSolver("cholesky") beside
// ReducedSystem("explicit") or NormalMatrix("explicit"), emitted only for energies with the
// statement (the factorisation and the solves themselves are not generated: dense_cholesky.hip).
//   gen_dense_fill   one workgroup per block-CSR block with column <= row: the C x C block to
//                    its place in the 64 x 64 tiles of the dense lower triangle (tile (I, J) at
//                    (I (I + 1) / 2 + J) 64^2, row-major inside; the caller zeroes the tiles
//                    first). LM's clamped diagonal (dadd, the SpMV's) is added to the diagonal;
//                    the rows and columns of inactive elements become identity rows with
//                    right-hand side 0. The diagonal block's workgroup also writes the row's
//                    original diagonal (the pivot rule's reference) and its entries of the
//                    right-hand side, gathered from the unknown vector's layout into element-major
//                    order; workgroup 0 the padding up to a multiple of 64 (diagonal 1, right-hand
//                    side 0). Whole blocks, one writer per entry, no atomics.
//   gen_dense_store  the solution back to the retained unknowns' places of delta; inactive
//                    elements keep their 0. Returns at entry when the factorisation failed.
// Both read the channels' places through opt_rbase / opt_rstride (emit_group_rows).
#include "codegen_ctx.h"

namespace optamd {
namespace gen {

void emit_dense(Ctx& cx, std::ostringstream& o, const std::string& Gr, int C) {
    if (!cx.m.direct_cholesky) return;
    cx.gs.has_dense = true;
    o << "extern \"C\" __global__ __launch_bounds__(256) void gen_dense_fill(GenArgs a, const int* __restrict__ blkRow,\n"
         "        const int* __restrict__ colInd, const T* __restrict__ val, long long nnzb, const T* __restrict__ dadd,\n"
         "        const T* __restrict__ r, T* __restrict__ tiles, T* __restrict__ diag0, T* __restrict__ rhs) {\n"
         "    constexpr int C = " << C << ", CC = C * C;\n"
         "    const int t = threadIdx.x;\n"
         "    for (long long b = blockIdx.x; b < nnzb; b += gridDim.x) {\n"
         "        const long long row = blkRow[b], col = colInd[b];\n"
         "        if (col > row) continue;\n"
         "        const bool on = " << Gr << "::act(a, row) && " << Gr << "::act(a, col);\n"
         "        for (int ij = t; ij < CC; ij += 256) {\n"
         "            const int i = ij / C, j = ij - i * C;\n"
         "            const long long gi = row * C + i, gj = col * C + j, I = gi >> 6, J = gj >> 6;\n"
         "            if (J > I) continue;   // (a diagonal block across a tile boundary: its upper part)\n"
         "            const bool dg = row == col && i == j;\n"
         "            const long long x = opt_rbase(a, i) + row * opt_rstride(i);\n"
         "            T v = on ? val[b * CC + ij] : (dg ? (T)1 : (T)0);\n"
         "            if (on && dg && dadd) v += dadd[x];\n"
         "            tiles[(I * (I + 1) / 2 + J) * 4096 + (gi & 63) * 64 + (gj & 63)] = v;\n"
         "            if (dg) {\n"
         "                diag0[gi] = v;\n"
         "                rhs[gi] = on ? r[x] : (T)0;\n"
         "            }\n"
         "        }\n"
         "    }\n"
         "    if (blockIdx.x == 0) {\n"
         "        const long long n = " << Gr << "::n(a) * C, np = ((n + 63) >> 6) << 6;\n"
         "        for (long long gi = n + t; gi < np; gi += 256) {\n"
         "            const long long I = gi >> 6;\n"
         "            tiles[(I * (I + 1) / 2 + I) * 4096 + (gi & 63) * 65] = (T)1;\n"
         "            diag0[gi] = (T)1;\n"
         "            rhs[gi] = (T)0;\n"
         "        }\n"
         "    }\n"
         "}\n";
    o << "extern \"C\" __global__ __launch_bounds__(256) void gen_dense_store(GenArgs a, const T* __restrict__ x,\n"
         "        T* __restrict__ delta, const int* __restrict__ fail) {\n"
         "    if (*fail >= 0) return;\n"
         "    constexpr int C = " << C << ";\n"
         "    const long long n = " << Gr << "::n(a) * C;\n"
         "    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {\n"
         "        const long long row = e / C;\n"
         "        const int i = (int)(e - row * C);\n"
         "        if (" << Gr << "::act(a, row)) delta[opt_rbase(a, i) + row * opt_rstride(i)] = x[e];\n"
         "    }\n"
         "}\n";
}

}  // namespace gen
}  // namespace optamd
