// gen/codegen_schur_explicit.cpp — the explicitly formed Schur complement's kernels
// (ReducedSystem("explicit") beside Eliminate), emitted only for energies with the statement.
//
// S = B - E M^-1 E^T over the retained group (one index space, Cr channels per element) is kept
// in block-CSR with Cr x Cr blocks. An edge instance q — one edge of one graph seen from its
// eliminated vertex p and one retained slot's vertex c — contributes W_q = sum over the edge's
// residuals of g_retained (x) g_eliminated (Cr x Ce) to E's block (c, p), so
//   S(c1, c2) = [c1 = c2] B_c1 - sum over p, over pairs (q1, q2) at p with c(q1) = c1, c(q2) = c2
//               of Y_q1 W_q2^T,      Y_q = W_q M_p^-1.
// The pattern and every block's pair list come from the host (schur_pattern.h), in a fixed order.
//   gen_schur_eblk      generated. Per eliminated vertex (one lane, the walk of gen_schur_elim):
//                       M_p^-1 once, then W_q and Y_q of every incident instance, written at the
//                       instance's position (list base + index in the incidence order)
//   gen_schur_assemble  hand-written. One wave per block of S, one lane per entry (i, j), a
//                       wave-uniform loop over the block's pairs in list order: the lanes of a
//                       wave read Y_q1 and W_q2 as two contiguous runs of Cr Ce values. B_c comes
//                       from the packed blocks gen_jtf / gen_jtf_graph left (before gen_blk_init
//                       inverts them). No atomics: one wave owns a block. Blocks with more than
//                       kSchurLongPairs pairs (the hubs' diagonal blocks) go to
//                       gen_schur_assemble_long: one workgroup per block, the list dealt to
//                       256 / Cr^2 slices whose sums meet in LDS in slice order
//   gen_schur_spmv      hand-written. One workgroup per block row; the row's values are one
//                       contiguous run, read by consecutive lanes (lane = (block in pass, i, j),
//                       256 / Cr^2 blocks per pass), each lane keeping its (i, j) for the whole
//                       row; the lanes' partial sums meet in LDS and channel i adds them in lane
//                       order. The contract of gen_schur_apply: early return on *stop, 0 in the
//                       rows of inactive elements, columns unmasked, + dadd p, 0 into the
//                       eliminated part of Ap, p.Ap through block_reduce_publish
// Cr, Ce and the channels' places in the unknown vector are literals, as for gen_blk_*: the
// kernels live in the energy's module beside GenArgs, ReduceSlot and the group structs.
#include <algorithm>
#include "codegen_ctx.h"

namespace optamd {
namespace gen {

// The assembly of a block-CSR matrix whose block b is [row = col] B_row (+ or -) the sum over the
// block's pair list of Y_q1 W_q2^T (Y, W: CR x CE per instance): `name` sums a block with one
// wave, one lane per entry, `name`_long the blocks with more than kSchurLongPairs pairs (listed by
// the host) with one workgroup each. minus: the Schur complement's sign; the explicitly formed
// J^T J (codegen_normal.cpp) adds, with Y = W. Gr: the block group B is packed for.
// packed: a wave sums 64 / CR^2 blocks at once, lane = (block in the wave, entry), each lane
// walking its own block's list (J^T J has millions of blocks of two or three pairs; a wave per
// block leaves most lanes idle). The order inside an entry's sum is the list's either way.
void emit_pair_assemble(std::ostringstream& o, const std::string& name, int CR, int CE, const std::string& Gr, bool minus,
                        bool packed) {
    const char* sign = minus ? "-" : "+";
    if (packed)
        o << "extern \"C\" __global__ __launch_bounds__(256) void " << name << "(GenArgs a, const T* __restrict__ blk,\n"
             "        const T* __restrict__ Wq, const T* __restrict__ Yq, const int* __restrict__ blkRow, const int* __restrict__ colInd,\n"
             "        const int* __restrict__ pairPtr, const int* __restrict__ pairs, T* __restrict__ val, int nnzb) {\n"
             "    constexpr int CR = " << CR << ", CE = " << CE << ", CC = CR * CR, CW = CR * CE, NBW = 64 / CC;\n"
             "    const int lane = threadIdx.x & 63;\n"
             "    const int bl = lane / CC, ij = lane - bl * CC, i = ij / CR, j = ij - i * CR;\n"
             "    const long long bN = " << Gr << "::n(a), bB = " << Gr << "::base(a);\n"
             "    const int tij = i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i;\n"
             "    const long long nw = ((long long)nnzb + NBW - 1) / NBW;\n"
             "    for (long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); g < nw; g += (long long)gridDim.x * 4) {\n"
             "        const long long b = g * NBW + bl;\n"
             "        if (bl >= NBW || b >= nnzb) continue;\n"
             "        const int row = blkRow[b], col = colInd[b];\n"
             "        const int p0 = pairPtr[b], p1 = pairPtr[b + 1];\n"
             "        if (p1 - p0 > " << kSchurLongPairs << ") continue;   // " << name << "_long's\n"
             "        T acc = row == col ? blk[bB + (long long)tij * bN + row] : (T)0;\n"
             "#pragma unroll 4\n"
             "        for (int pp = p0; pp < p1; ++pp) {\n"
             "            const int q1 = pairs[2LL * pp], q2 = pairs[2LL * pp + 1];\n"
             "            const T* y = Yq + (long long)q1 * CW + i * CE;\n"
             "            const T* w = Wq + (long long)q2 * CW + j * CE;\n"
             "            T s = y[0] * w[0];\n"
             "#pragma unroll\n"
             "            for (int c = 1; c < CE; ++c) s += y[c] * w[c];\n"
             "            acc " << sign << "= s;\n"
             "        }\n"
             "        val[b * CC + ij] = acc;\n"
             "    }\n"
             "}\n";
    else
    o << "extern \"C\" __global__ __launch_bounds__(256) void " << name << "(GenArgs a, const T* __restrict__ blk,\n"
         "        const T* __restrict__ Wq, const T* __restrict__ Yq, const int* __restrict__ blkRow, const int* __restrict__ colInd,\n"
         "        const int* __restrict__ pairPtr, const int* __restrict__ pairs, T* __restrict__ val, int nnzb) {\n"
         "    constexpr int CR = " << CR << ", CE = " << CE << ", CC = CR * CR, CW = CR * CE;\n"
         "    const int lane = threadIdx.x & 63;\n"
         "    const int i = lane / CR, j = lane - i * CR;\n"
         "    const bool on = lane < CC;\n"
         "    const long long bN = " << Gr << "::n(a), bB = " << Gr << "::base(a);\n"
         "    const int tij = i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i;\n"
         "    for (long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); b < nnzb; b += (long long)gridDim.x * 4) {\n"
         "        const int row = blkRow[b], col = colInd[b];\n"
         "        const int p0 = pairPtr[b], p1 = pairPtr[b + 1];\n"
         "        if (p1 - p0 > " << kSchurLongPairs << ") continue;   // " << name << "_long's\n"
         "        T acc = (on && row == col) ? blk[bB + (long long)tij * bN + row] : (T)0;\n"
         "        if (on) {\n"
         "#pragma unroll 4\n"
         "            for (int pp = p0; pp < p1; ++pp) {\n"
         "                const int q1 = pairs[2LL * pp], q2 = pairs[2LL * pp + 1];\n"
         "                const T* y = Yq + (long long)q1 * CW + i * CE;\n"
         "                const T* w = Wq + (long long)q2 * CW + j * CE;\n"
         "                T s = y[0] * w[0];\n"
         "#pragma unroll\n"
         "                for (int c = 1; c < CE; ++c) s += y[c] * w[c];\n"
         "                acc " << sign << "= s;\n"
         "            }\n"
         "            val[b * CC + lane] = acc;\n"
         "        }\n"
         "    }\n"
         "}\n";

    // the blocks with long lists (the hubs' diagonal blocks: one pair per observation), listed by
    // the host: one workgroup per block, the list dealt to 256 / Cr^2 slices of Cr^2 lanes, the
    // slices' sums subtracted from (or added to) B in slice order through LDS
    o << "extern \"C\" __global__ __launch_bounds__(256) void " << name << "_long(GenArgs a, const T* __restrict__ blk,\n"
         "        const T* __restrict__ Wq, const T* __restrict__ Yq, const int* __restrict__ blkRow, const int* __restrict__ colInd,\n"
         "        const int* __restrict__ pairPtr, const int* __restrict__ pairs, T* __restrict__ val,\n"
         "        const int* __restrict__ longBlk, int nlong) {\n"
         "    constexpr int CR = " << CR << ", CE = " << CE << ", CC = CR * CR, CW = CR * CE, NS = 256 / CC;\n"
         "    __shared__ T part[256];\n"
         "    const int t = threadIdx.x;\n"
         "    const int sl = t / CC, ij = t - sl * CC, i = ij / CR, j = ij - i * CR;\n"
         "    const long long bN = " << Gr << "::n(a), bB = " << Gr << "::base(a);\n"
         "    const int tij = i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i;\n"
         "    for (int k = blockIdx.x; k < nlong; k += gridDim.x) {\n"
         "        const int b = longBlk[k];\n"
         "        const int row = blkRow[b], col = colInd[b];\n"
         "        const int p0 = pairPtr[b], p1 = pairPtr[b + 1];\n"
         "        T acc = 0;\n"
         "        if (sl < NS) {\n"
         "#pragma unroll 4\n"
         "            for (int pp = p0 + sl; pp < p1; pp += NS) {\n"
         "                const int q1 = pairs[2LL * pp], q2 = pairs[2LL * pp + 1];\n"
         "                const T* y = Yq + (long long)q1 * CW + i * CE;\n"
         "                const T* w = Wq + (long long)q2 * CW + j * CE;\n"
         "                T s = y[0] * w[0];\n"
         "#pragma unroll\n"
         "                for (int c = 1; c < CE; ++c) s += y[c] * w[c];\n"
         "                acc += s;\n"
         "            }\n"
         "        }\n"
         "        part[t] = acc;\n"
         "        __syncthreads();\n"
         "        if (t < CC) {\n"
         "            T s = row == col ? blk[bB + (long long)tij * bN + row] : (T)0;\n"
         "            for (int h = 0; h < NS; ++h) s " << sign << "= part[h * CC + t];\n"
         "            val[(long long)b * CC + t] = s;\n"
         "        }\n"
         "        __syncthreads();\n"
         "    }\n"
         "}\n";
}

// the place of block row j of group GR in the unknown vector: element e's value is at
// opt_rbase(a, j) + e * opt_rstride(j)
void emit_group_rows(const Ctx& cx, std::ostringstream& o, const GBlockGroup& GR) {
    const GModel& m = cx.m;
    o << "__device__ __forceinline__ long long opt_rbase(const GenArgs& a, int j) {\n    return ";
    for (size_t q = 0; q < GR.images.size(); ++q) {
        const int k = GR.images[q];
        if (q + 1 < GR.images.size()) o << "j < " << GR.first_row[q] + m.images[k].channels << " ? ";
        o << "a.uoff[" << cx.uslot[k] << "] + (j - " << GR.first_row[q] << ")";
        if (q + 1 < GR.images.size()) o << " : ";
    }
    o << ";\n}\n__device__ __forceinline__ int opt_rstride(int j) {\n    return ";
    for (size_t q = 0; q < GR.images.size(); ++q) {
        const int k = GR.images[q];
        if (q + 1 < GR.images.size()) o << "j < " << GR.first_row[q] + m.images[k].channels << " ? ";
        o << m.images[k].channels;
        if (q + 1 < GR.images.size()) o << " : ";
    }
    o << ";\n}\n";
}

void emit_schur_explicit(Ctx& cx, std::ostringstream& o) {
    if (!cx.schur() || !cx.m.reduced_explicit || !explicit_refusal(cx.m).empty()) return;
    GModel& m = cx.m;
    Pool& P = cx.P;
    GenSource& gs = cx.gs;
    const int eg = cx.elim_group, es = cx.elim_space();
    int rg = -1;
    for (size_t g = 0; g < cx.groups.size(); ++g)
        if ((int)g != eg) rg = (int)g;
    const GBlockGroup &GE = cx.groups[eg], &GR = cx.groups[rg];
    const int CR = GR.C, CE = GE.C;
    const std::string Ge = "OptGroup" + std::to_string(eg), Gr = "OptGroup" + std::to_string(rg);
    const std::string ess = std::to_string(es);
    gs.has_schur_explicit = true;
    gs.schur_cr = CR;
    gs.schur_ce = CE;
    gs.schur_rspace = GR.space;

    // ------------------------------------------------------------------ gen_schur_eblk
    o << "struct OptQBase { long long b[16]; };   // first position of each instance list\n";
    o << "extern \"C\" __global__ __launch_bounds__(256) void gen_schur_eblk(GenArgs a, const T* __restrict__ blk,\n"
         "        T* __restrict__ Wq, T* __restrict__ Yq, OptQBase qb) {\n"
         "    typedef " << Ge << " G;\n"
         "    constexpr int C = G::C;\n"
         "    {\n    const int W = a.sdims[" << ess << "][0], H = a.sdims[" << ess << "][1], D = a.sdims[" << ess << "][2]; (void)W; (void)H; (void)D;\n"
         "    for (long long vtx = opt_xcd_block() * 256 + threadIdx.x; vtx < a.snpix[" << ess << "]; vtx += (long long)gridDim.x * 256) {\n"
         "        T m[C * (C + 1) / 2];\n"
         "        opt_blk_load<G>(a, blk, vtx, m);\n";
    for (size_t g = 0; g < m.graphs.size(); ++g) {
        const size_t nslots = m.graphs[g].slot_names.size();
        for (size_t k = 0; k < nslots; ++k) {
            if (m.graphs[g].slot_space[k] != es) continue;
            // the retained slots of the residuals that read the group at slot k
            std::vector<int> rslots;
            for (auto& r : m.residuals) {
                if (r.graph != (int)g) continue;
                bool mine = false;
                for (int u : r.unknowns) mine |= m.is_eliminated(P.at(u).i) && P.at(u).slot == (int)k;
                for (int u : r.unknowns)
                    if (mine && !m.is_eliminated(P.at(u).i) &&
                        std::find(rslots.begin(), rslots.end(), P.at(u).slot) == rslots.end())
                        rslots.push_back(P.at(u).slot);
            }
            if (rslots.empty()) continue;
            std::sort(rslots.begin(), rslots.end());
            const int sbk = gs.slot_base[g] + (int)k;
            std::vector<int> list_of(nslots, -1);
            for (int rs : rslots) {
                list_of[rs] = (int)gs.schur_lists.size();
                gs.schur_lists.push_back({(int)g, sbk, gs.slot_base[g] + rs});
            }
            std::ostringstream pre, body, decl, tail;
            Body b(cx, body, cx.nd_of(es));
            b.hoist_to(&pre, (int)k, (int)g);
            if (cx.has_loss()) b.weight_at(cx.weight_at_q(sbk));
            for (int rs : rslots) {
                decl << "        T";
                for (int i = 0; i < CR; ++i)
                    for (int j = 0; j < CE; ++j)
                        decl << (i + j ? "," : "") << " w" << list_of[rs] << "_" << i << "_" << j << " = 0";
                decl << ";\n";
            }
            for (auto& r : m.residuals) {
                if (r.graph != (int)g) continue;
                std::vector<std::pair<std::string, int>> ge;   // (partial, block row) at the eliminated vertex
                for (int u : r.unknowns) {
                    const Node n = P.at(u);
                    if (!m.is_eliminated(n.i) || n.slot != (int)k) continue;
                    const int gu = P.diff(r.expr, u);
                    double gv;
                    if (P.is_const(gu, &gv) && gv == 0.0) continue;
                    ge.push_back({b.v(gu), cx.blk_row(eg, n.i, n.ch)});
                }
                if (ge.empty()) continue;
                for (int u : r.unknowns) {
                    const Node n = P.at(u);
                    if (m.is_eliminated(n.i)) continue;
                    const int gu = P.diff(r.expr, u);
                    double gv;
                    if (P.is_const(gu, &gv) && gv == 0.0) continue;
                    const std::string gr = b.v(gu);
                    const int row = cx.blk_row(rg, n.i, n.ch);
                    for (auto& e : ge)
                        b.line("w" + std::to_string(list_of[n.slot]) + "_" + std::to_string(row) + "_" +
                               std::to_string(e.second) + " += " + gr + " * " + e.first + ";");
                }
            }
            for (int rs : rslots) {
                const std::string l = std::to_string(list_of[rs]);
                tail << "        { const long long qi = (qb.b[" << l << "] + q) * " << CR * CE << ";\n";
                for (int i = 0; i < CR; ++i)
                    for (int j = 0; j < CE; ++j) {
                        std::string y;
                        for (int c = 0; c < CE; ++c)
                            y += std::string(c ? " + " : "") + "w" + l + "_" + std::to_string(i) + "_" + std::to_string(c) +
                                 " * m[" + std::to_string(tri(c, j)) + "]";
                        tail << "          Wq[qi + " << i * CE + j << "] = w" << l << "_" << i << "_" << j << "; Yq[qi + "
                             << i * CE + j << "] = " << y << ";\n";
                    }
                tail << "        }\n";
            }
            // the other slots' vertices, as graph_gather reads them
            std::ostringstream loop;
            for (size_t s2 = 0; s2 < nslots; ++s2)
                if (s2 != k) {
                    const std::pair<int, int> key(sbk, gs.slot_base[g] + (int)s2);
                    auto it = std::find(gs.nb_pairs.begin(), gs.nb_pairs.end(), key);
                    const int idx = (int)(it - gs.nb_pairs.begin());
                    if (it == gs.nb_pairs.end()) gs.nb_pairs.push_back(key);
                    const std::string gnb = "a.gnb[" + std::to_string(idx) + "]";
                    if (idx < 32)
                        loop << "        const int v" << s2 << " = "
                             << (cx.off32 ? "opt_g32(" + gnb + ", q, 1, 0)" : gnb + "[q]") << ";\n";
                    else
                        loop << "        const int v" << s2 << " = a.slot[" << key.second << "][a.geid[" << sbk << "][q]];\n";
                }
            o << "        {\n        const int v" << k << " = (int)vtx;\n" << pre.str()
              << "        const int q0 = a.goff[" << sbk << "][vtx], q1 = a.goff[" << sbk << "][vtx + 1];\n"
              << "        for (int q = q0; q < q1; ++q) {\n" << loop.str() << decl.str() << body.str()
              << tail.str() << "        }\n        }\n";
        }
    }
    o << "    }\n    }\n}\n";

    emit_group_rows(cx, o, GR);

    // ------------------------------------------------------------------ gen_schur_assemble
    emit_pair_assemble(o, "gen_schur_assemble", CR, CE, Gr, true);

    // ------------------------------------------------------------------ gen_schur_spmv
    o << "extern \"C\" __global__ __launch_bounds__(256) void gen_schur_spmv(GenArgs a, const int* __restrict__ rowPtr,\n"
         "        const int* __restrict__ colInd, const T* __restrict__ val, const T* __restrict__ p, T* __restrict__ Ap,\n"
         "        const T* __restrict__ dadd, const int* stop, ReduceSlot rs) {\n"
         "    if (stop && *stop) return;\n"
         "    constexpr int CR = " << CR << ", CC = CR * CR, NB = 256 / CC;\n"
         "    __shared__ T part[256];\n"
         "    const int t = threadIdx.x;\n"
         "    const int bl = t / CC, ij = t - bl * CC, i = ij / CR, j = ij - i * CR; (void)i;\n"
         "    const bool on = bl < NB;\n"
         "    const long long pb = opt_rbase(a, j), ob = opt_rbase(a, t < CR ? t : 0);\n"
         "    const int pc = opt_rstride(j), oc = opt_rstride(t < CR ? t : 0);\n"
         "    const long long nR = " << Gr << "::n(a);\n"
         "    T dot = 0;\n"
         "    for (long long row = blockIdx.x; row < nR; row += gridDim.x) {\n"
         "        const int b0 = rowPtr[row], b1 = rowPtr[row + 1];\n"
         "        T acc = 0;\n"
         "        if (on) {\n"
         "#pragma unroll 4\n"
         "            for (int b = b0 + bl; b < b1; b += NB)\n"
         "                acc += val[(long long)b * CC + ij] * p[pb + (long long)colInd[b] * pc];\n"
         "        }\n"
         "        part[t] = acc;\n"
         "        __syncthreads();\n"
         "        if (t < CR) {\n"
         "            T s = 0;\n"
         "            for (int k = 0; k < NB; ++k)\n"
         "#pragma unroll\n"
         "                for (int c = 0; c < CR; ++c) s += part[k * CC + t * CR + c];\n"
         "            const long long x = ob + row * oc;\n"
         "            const T pe = p[x];\n"
         "            const T ov = " << Gr << "::act(a, row) ? s + (dadd ? dadd[x] * pe : (T)0) : (T)0;\n"
         "            Ap[x] = ov;\n"
         "            dot += pe * ov;\n"
         "        }\n"
         "        __syncthreads();\n"
         "    }\n"
         "    {\n    constexpr int C = " << Ge << "::C;\n"
         "    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < " << Ge << "::n(a); e += (long long)gridDim.x * 256) {\n"
         "        long long x[C];\n"
         "        " << Ge << "::ix(a, e, x);\n"
         "#pragma unroll\n"
         "        for (int c = 0; c < C; ++c) Ap[x[c]] = (T)0;\n"
         "    }\n    }\n"
         "    double v[1] = {(double)dot};\n    block_reduce_publish<1>(v, rs, blockIdx.x);\n}\n";
    emit_dense(cx, o, Gr, CR);
}

}  // namespace gen
}  // namespace optamd
