// gen/codegen_normal.cpp — the explicitly formed normal matrix's kernels (NormalMatrix("explicit")),
// emitted only for energies with the statement.
//
// H = J^T J over the one block group (one index space, C channels per element) is kept in
// block-CSR with C x C blocks. An edge instance q — one edge of one graph seen from one slot over
// the unknowns' space, at vertex v(q) — carries G_q, the C x R matrix of the edge's R residuals'
// partials with respect to that slot's channels, so
//   H(c1, c2) = [c1 = c2] B_c1 + sum over edges, over pairs (q1, q2) of two different instances
//               of the edge with v(q1) = c1, v(q2) = c2, of G_q1 G_q2^T,
// B_c the packed diagonal block gen_jtf / gen_jtf_graph leave (the centred terms, which read
// the unknowns at offset 0 only, and every instance's product with itself). The pattern and
// every block's pair list come from the host (schur_pattern.h, `distinct`), in a fixed order.
//   gen_normal_eblk      generated. One lane per edge: the edge's vertices, every residual's
//                        partials once, G_q of each of its instances written at the instance's
//                        position (list base + edge), zeros included
//   gen_normal_assemble  the pair-list assembly of codegen_schur_explicit.cpp with Y = W = G and
//                        the sums added, in its packed form: 64 / C^2 blocks per wave, one lane
//                        per entry, pairs in list order; blocks with more than kSchurLongPairs
//                        pairs (parallel edges) by gen_normal_assemble_long, one workgroup each.
//                        No atomics
//   gen_normal_spmv      hand-written, PCG's apply. Short rows (a pose has a handful of
//                        neighbours): C lanes serve one block row, lane = (row within the wave,
//                        channel i), a wave 64 / C rows; each lane walks its row's blocks in
//                        colInd order and adds H[b][i][j] p[col][j] in that order, the loop
//                        unrolled four blocks deep so that their loads are in flight together.
//                        The C lanes of a row read one block as one contiguous run of C^2
//                        values. No LDS, no atomics. Rows with more than kNormalLongRow blocks,
//                        listed by the host, are left out there and summed after it by whole
//                        workgroups, the row loop of gen_schur_spmv. The contract of
//                        gen_schur_spmv: early return on *stop, 0 in the rows of inactive
//                        elements, columns unmasked, + dadd p, p.Ap through block_reduce_publish
// C, R and the channels' places in the unknown vector are literals, as for gen_blk_*.
#include <algorithm>
#include "codegen_ctx.h"

namespace optamd {
namespace gen {

void emit_normal(Ctx& cx, std::ostringstream& o) {
    if (!cx.m.normal_explicit || cx.schur() || !cx.blockpre || !normal_refusal(cx.m).empty()) return;
    GModel& m = cx.m;
    Pool& P = cx.P;
    GenSource& gs = cx.gs;
    const GBlockGroup& GR = cx.groups[0];
    const int C = GR.C, us = GR.space;
    const std::string Gr = "OptGroup0";

    // the instance lists: per graph, the slots through which a residual reads an unknown
    std::vector<std::vector<int>> list_of(m.graphs.size());
    std::vector<int> nres(m.graphs.size(), 0);
    int R = 1;
    for (size_t g = 0; g < m.graphs.size(); ++g) {
        const size_t nslots = m.graphs[g].slot_names.size();
        list_of[g].assign(nslots, -1);
        std::vector<bool> reads(nslots, false);
        for (auto& r : m.residuals) {
            if (r.graph != (int)g) continue;
            ++nres[g];
            for (int u : r.unknowns)
                if (P.at(u).slot >= 0) reads[P.at(u).slot] = true;
        }
        for (size_t k = 0; k < nslots; ++k)
            if (reads[k] && (!cx.mspace || m.graphs[g].slot_space[k] == us)) {
                list_of[g][k] = (int)gs.normal_lists.size();
                gs.normal_lists.push_back({(int)g, gs.slot_base[g] + (int)k});
                R = std::max(R, nres[g]);
            }
    }
    gs.has_normal = true;
    gs.normal_c = C;
    gs.normal_r = R;
    gs.normal_space = us;

    // ------------------------------------------------------------------ gen_normal_eblk
    o << "struct OptQBase { long long b[16]; };   // first position of each instance list\n";
    o << "extern \"C\" __global__ __launch_bounds__(256) void gen_normal_eblk(GenArgs a, T* __restrict__ Gq, OptQBase qb) {\n"
      << cx.top_coords();
    for (size_t g = 0; g < m.graphs.size(); ++g) {
        bool any = false;
        for (int l : list_of[g]) any |= l >= 0;
        if (!any) continue;
        const size_t nslots = m.graphs[g].slot_names.size();
        o << "    {\n    const long long es = (long long)gridDim.x * 256, ne = a.nedge[" << g << "];\n"
          << "    for (long long e = opt_xcd_block() * 256 + threadIdx.x; e < ne; e += es) {\n";
        for (size_t s = 0; s < nslots; ++s)
            o << "        const int v" << s << " = a.slot[" << gs.slot_base[g] + s << "][e];\n";
        std::ostringstream body;
        Body b(cx, body, cx.nd);
        if (cx.has_loss()) b.weight_at(cx.weight_at_e());
        // entry (row, residual) of each list's G: the partial's temporary, "" = 0
        std::vector<std::vector<std::string>> G(nslots, std::vector<std::string>((size_t)C * R));
        int rho = 0;
        for (auto& r : m.residuals) {
            if (r.graph != (int)g) continue;
            for (int u : r.unknowns) {
                const Node n = P.at(u);
                if (n.slot < 0 || list_of[g][n.slot] < 0) continue;
                const int gu = P.diff(r.expr, u);
                double gv;
                if (P.is_const(gu, &gv) && gv == 0.0) continue;
                G[n.slot][(size_t)cx.blk_row(0, n.i, n.ch) * R + rho] = b.v(gu);
            }
            ++rho;
        }
        o << body.str();
        for (size_t k = 0; k < nslots; ++k) {
            if (list_of[g][k] < 0) continue;
            o << "        { T* gq = Gq + (qb.b[" << list_of[g][k] << "] + e) * " << C * R << ";\n";
            for (int x = 0; x < C * R; ++x)
                o << "          gq[" << x << "] = " << (G[k][x].empty() ? "(T)0" : G[k][x]) << ";\n";
            o << "        }\n";
        }
        o << "    }\n    }\n";
    }
    o << "}\n";

    emit_group_rows(cx, o, GR);

    // ------------------------------------------------------------------ gen_normal_assemble
    emit_pair_assemble(o, "gen_normal_assemble", C, R, Gr, false, true);

    // ------------------------------------------------------------------ gen_normal_spmv
    o << "extern \"C\" __global__ __launch_bounds__(256) void gen_normal_spmv(GenArgs a, const int* __restrict__ rowPtr,\n"
         "        const int* __restrict__ colInd, const T* __restrict__ val, const T* __restrict__ p, T* __restrict__ Ap,\n"
         "        const T* __restrict__ dadd, const int* stop, ReduceSlot rs, const int* __restrict__ longRow, int nlong) {\n"
         "    if (stop && *stop) return;\n"
         "    constexpr int C = " << C << ", CC = C * C, RW = 64 / C, RB = 4 * RW, LONG = " << kNormalLongRow << ";\n"
         "    const int t = threadIdx.x;\n"
         "    const long long nR = " << Gr << "::n(a);\n"
         "    T dot = 0;\n"
         "    {   // short rows: C lanes per row, 64 / C rows per wave, XCD-contiguous groups of 4 waves' rows\n"
         "    const int lane = t & 63, rl = lane / C, i = lane - rl * C;\n"
         "    const long long ob = opt_rbase(a, i);\n"
         "    const int oc = opt_rstride(i);\n"
         "    const long long ngrp = (nR + RB - 1) / RB;\n"
         "    for (long long g = opt_xcd_block(); g < ngrp; g += gridDim.x) {\n"
         "        const long long row = g * RB + (t >> 6) * RW + rl;\n"
         "        if (rl >= RW || row >= nR) continue;\n"
         "        const int b0 = rowPtr[row], b1 = rowPtr[row + 1];\n"
         "        if (b1 - b0 > LONG) continue;   // the workgroup form's, below\n"
         "        T acc = 0;\n"
         "        const T* hrow = val + (long long)b0 * CC + i * C;   // the row's run; 32-bit offsets inside it\n"
         "        const int* crow = colInd + b0;\n"
         "        const int nb = b1 - b0;\n"
         "#pragma unroll 4\n"
         "        for (int k = 0; k < nb; ++k) {\n"
         "            const long long col = crow[k];\n"
         "            const T* h = hrow + k * CC;\n"
         "#pragma unroll\n"
         "            for (int j = 0; j < C; ++j) acc += h[j] * p[opt_rbase(a, j) + col * opt_rstride(j)];\n"
         "        }\n"
         "        const long long x = ob + row * oc;\n"
         "        const T pe = p[x];\n"
         "        const T ov = " << Gr << "::act(a, row) ? acc + (dadd ? dadd[x] * pe : (T)0) : (T)0;\n"
         "        Ap[x] = ov;\n"
         "        dot += pe * ov;\n"
         "    }\n"
         "    }\n"
         "    if (nlong > 0) {   // long rows: one workgroup per row (gen_schur_spmv's row loop)\n"
         "        constexpr int NB = 256 / CC;\n"
         "        __shared__ T part[256];\n"
         "        const int bl = t / CC, ij = t - bl * CC, i = ij / C, j = ij - i * C; (void)i;\n"
         "        const bool on = bl < NB;\n"
         "        const long long pb = opt_rbase(a, j), ob = opt_rbase(a, t < C ? t : 0);\n"
         "        const int pc = opt_rstride(j), oc = opt_rstride(t < C ? t : 0);\n"
         "        for (int k = blockIdx.x; k < nlong; k += gridDim.x) {\n"
         "            const long long row = longRow[k];\n"
         "            const int b0 = rowPtr[row], b1 = rowPtr[row + 1];\n"
         "            T acc = 0;\n"
         "            if (on) {\n"
         "#pragma unroll 2\n"
         "                for (int b = b0 + bl; b < b1; b += NB)\n"
         "                    acc += val[(long long)b * CC + ij] * p[pb + (long long)colInd[b] * pc];\n"
         "            }\n"
         "            part[t] = acc;\n"
         "            __syncthreads();\n"
         "            if (t < C) {\n"
         "                T s = 0;\n"
         "#pragma unroll 2\n"
         "                for (int h = 0; h < NB; ++h)   // (fully unrolled, its 256 / C LDS reads in flight set the kernel's VGPRs)\n"
         "#pragma unroll\n"
         "                    for (int c = 0; c < C; ++c) s += part[h * CC + t * C + c];\n"
         "                const long long x = ob + row * oc;\n"
         "                const T pe = p[x];\n"
         "                const T ov = " << Gr << "::act(a, row) ? s + (dadd ? dadd[x] * pe : (T)0) : (T)0;\n"
         "                Ap[x] = ov;\n"
         "                dot += pe * ov;\n"
         "            }\n"
         "            __syncthreads();\n"
         "        }\n"
         "    }\n"
         "    double v[1] = {(double)dot};\n    block_reduce_publish<1>(v, rs, blockIdx.x);\n}\n";
    emit_dense(cx, o, Gr, C);
}

}  // namespace gen
}  // namespace optamd
