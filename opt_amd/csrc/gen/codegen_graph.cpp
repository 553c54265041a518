// gen/codegen_graph.cpp — the graph gather kernels (gen_jtf_graph / gen_apply_graph) and the
// block preconditioner's PCG kernels (gen_blk_*).
#include <algorithm>
#include "codegen_ctx.h"

namespace optamd {
namespace gen {

// ------------------------------------------------------------- graph gathers
// The reference scatters every edge's J^T F / J^T J p contributions to the edge's
// vertices with float atomics (createjtfgraph / createjtjgraph, o.t:2833-2867,
// 2969-2994; Image:atomicAddChannel, backend_cuda.t:751-759). Here each vertex gathers
// them instead, over per-slot incidence lists built once per bind (a.goff / a.geid:
// the edges whose slot k is this vertex, ascending): no atomics, a fixed summation
// order (bitwise reproducible), each edge evaluated once per incident slot. The same
// kernel finishes the element (exclusion mask, LM diagonal, p.Ap).
// Several index spaces: the vertices of space sp gather through the slots that index sp
// (an unknown read at slot k lies over slot k's space, so only sp's unknowns accumulate);
// the other slots' vertices come from the gnb copies as before.
// schur (codegen_schur.cpp): 1 the sum J p takes the retained images only (u_e = (E^T p_r)_e
// at a vertex of the eliminated space); 2 it reads the eliminated images from "w"
void graph_gather(Ctx& cx, std::ostringstream& o, bool apply, int sp, int schur) {
    GModel& m = cx.m;
    Pool& P = cx.P;
    GenSource& gs = cx.gs;
    const std::vector<int>& uslot = cx.uslot;
    const bool prefetch_nb = cx.knobs.prefetch_nb;
    const std::string unroll = cx.knobs.edge_unroll > 1 ? "#pragma unroll " + std::to_string(cx.knobs.edge_unroll) + "\n" : "";
    // accumulators per output (unknown image, channel)
    for (int k : cx.unk)
        for (int ch = 0; ch < m.images[k].channels && cx.in_space(k, sp); ++ch)
            o << "        T acc" << uslot[k] << "_" << ch << " = 0, dg" << uslot[k] << "_" << ch << " = 0;\n";
    const int bg = cx.blockpre && !apply ? cx.group_of(sp) : -1;
    for (int j = 0; bg >= 0 && j < cx.groups[bg].entries(); ++j) o << "        T bk" << j << " = 0;\n";
    o << "        (void)0;\n";
    for (size_t g = 0; g < m.graphs.size(); ++g) {
        const size_t nslots = m.graphs[g].slot_names.size();
        for (size_t k = 0; k < nslots; ++k) {
            // residuals of graph g reading an unknown at slot k
            bool any = false;
            for (auto& r : m.residuals)
                if (r.graph == (int)g)
                    for (int u : r.unknowns) any |= P.at(u).slot == (int)k;
            if (!any) continue;
            if (cx.mspace && m.graphs[g].slot_space[k] != sp) continue;
            const int sbk = gs.slot_base[g] + (int)k;
            std::ostringstream pre, body;
            Body b(cx, body, cx.nd_of(sp));   // (slot reads use no coordinates)
            b.hoist_to(&pre, (int)k, (int)g);
            // RobustEnergy: the group's weight at q, streaming beside the gnb copies (loading it one
            // edge ahead as the vertex ids are measured no gain: DESIGN.md §3.6)
            if (cx.has_loss()) b.weight_at(cx.weight_at_q(sbk));
            int idx = 0;
            for (auto& r : m.residuals) {
                if (r.graph != (int)g) continue;
                std::vector<int> mine;
                for (int u : r.unknowns)
                    if (P.at(u).slot == (int)k) mine.push_back(u);
                if (mine.empty()) continue;
                std::string R;
                if (apply) {
                    std::string sum = "(T)0";
                    for (int u : r.unknowns) {
                        const bool elim = schur && m.is_eliminated(P.at(u).i);
                        if (schur == 1 && elim) continue;
                        const int gu = P.diff(r.expr, u);
                        double gv;
                        if (P.is_const(gu, &gv) && gv == 0.0) continue;
                        sum += " + " + b.v(gu) + " * " + b.vec(u, schur == 2 && elim ? "w" : "p");
                    }
                    R = "jp" + std::to_string(idx++);
                    b.line("const T " + R + " = " + sum + ";");
                } else {
                    R = b.v(r.expr);
                }
                std::vector<std::pair<std::string, int>> own;   // (partial, block row) of this vertex's unknowns
                for (int u : mine) {
                    const int gu = P.diff(r.expr, u);
                    double gv;
                    if (P.is_const(gu, &gv) && gv == 0.0) continue;
                    const Node n = P.at(u);
                    const std::string gn = b.v(gu);
                    if (bg >= 0) {
                        own.push_back({gn, cx.blk_row(bg, n.i, n.ch)});
                        for (auto& w : own)
                            b.line("bk" + std::to_string(tri(own.back().second, w.second)) + " += " + gn + " * " + w.first + ";");
                    }
                    const std::string a_ = "acc" + std::to_string(uslot[n.i]) + "_" + std::to_string(n.ch);
                    const std::string d_ = "dg" + std::to_string(uslot[n.i]) + "_" + std::to_string(n.ch);
                    b.line(a_ + " += " + gn + " * " + R + ";" + (apply ? "" : " " + d_ + " += " + gn + " * " + gn + ";"));
                }
            }
            // { own-vertex values; for each incident edge { the other slots; the rest } }
            // the other slots' vertices come from per-incidence-order copies (one load
            // each instead of the edge id, then the slot array)
            // the next edge's other-slot vertex ids are loaded one edge ahead (prefetch_nb),
            // so an edge's gathers do not wait behind its id load
            std::ostringstream head, loop;
            for (size_t s2 = 0; s2 < nslots; ++s2)
                if (s2 != k) {
                    const std::pair<int, int> key(sbk, gs.slot_base[g] + (int)s2);
                    auto it = std::find(gs.nb_pairs.begin(), gs.nb_pairs.end(), key);
                    int idx = (int)(it - gs.nb_pairs.begin());
                    if (it == gs.nb_pairs.end()) gs.nb_pairs.push_back(key);
                    const std::string vs = "v" + std::to_string(s2), ns = "n" + std::to_string(s2);
                    const std::string gnb = "a.gnb[" + std::to_string(idx) + "]";
                    auto at = [&](const std::string& q) {
                        return cx.off32 ? "opt_g32(" + gnb + ", " + q + ", 1, 0)" : gnb + "[" + q + "]";
                    };
                    if (idx < 32 && prefetch_nb) {
                        head << "        int " << ns << " = q0 < q1 ? " << at("q0") << " : 0;\n";
                        loop << "        const int " << vs << " = " << ns << ";\n"
                             << "        if (q + 1 < q1) " << ns << " = " << at("q + 1") << ";\n";
                    } else if (idx < 32) {   // GenArgs::gnb capacity; past it, through the edge id
                        loop << "        const int " << vs << " = " << at("q") << ";\n";
                    } else {
                        loop << "        const int " << vs << " = a.slot[" << key.second << "][a.geid[" << sbk
                             << "][q]];\n";
                    }
                }
            o << "        {\n        const int v" << k << " = (int)vtx;\n" << pre.str()
              << "        const int q0 = a.goff[" << sbk << "][vtx], q1 = a.goff[" << sbk << "][vtx + 1];\n"
              << head.str() << unroll << "        for (int q = q0; q < q1; ++q) {\n" << loop.str();
            o << body.str() << "        }\n        }\n";
        }
    }
}

void emit_graph_gathers(Ctx& cx, std::ostringstream& o) {
    GModel& m = cx.m;
    GenSource& gs = cx.gs;
    const std::vector<int>& uslot = cx.uslot;
    // the vertex loop of a space and its flags
    auto open_vtx = [&](int sp) -> std::string {
        if (!cx.mspace)
            return "    for (long long vtx = opt_xcd_block() * 256 + threadIdx.x; vtx < a.npix; vtx += (long long)gridDim.x * 256) {\n";
        const std::string s = std::to_string(sp);
        return "    {\n    const long long fb = a.fbase[" + s + "];\n"
               "    for (long long vtx = opt_xcd_block() * 256 + threadIdx.x; vtx < a.snpix[" + s + "]; vtx += (long long)gridDim.x * 256) {\n";
    };
    const std::string vflag = cx.mspace ? "a.flags[fb + vtx]" : "a.flags[vtx]";
    o << "extern \"C\" __global__ __launch_bounds__(256) void gen_jtf_graph(GenArgs a, T* __restrict__ r, T* __restrict__ diag" << cx.blk_arg() << ") {\n"
      << cx.top_coords();
    for (int sp : cx.uspaces) {
        o << open_vtx(sp);
        graph_gather(cx, o, false, sp);
        o << "        const bool act = (" << vflag << " & 1) != 0;\n";
        for (int k : cx.unk)
            for (int ch = 0; ch < m.images[k].channels && cx.in_space(k, sp); ++ch) {
                const std::string e = "a.uoff[" + std::to_string(uslot[k]) + "] + vtx * " +
                                      std::to_string(m.images[k].channels) + " + " + std::to_string(ch);
                const std::string sfx = std::to_string(uslot[k]) + "_" + std::to_string(ch);
                o << "        { const long long i = " << e << "; r[i] = act ? r[i] - acc" << sfx
                  << " : (T)0; diag[i] += dg" << sfx << "; }\n";
            }
        if (cx.blockpre) {
            const int g = cx.group_of(sp);
            o << "        { const long long bN = " << cx.blk_n(g) << ", bB = " << cx.blk_base(g) << ";\n";
            for (int j = 0; j < cx.groups[g].entries(); ++j)
                o << "          blk[bB + " << j << "LL * bN + vtx] += bk" << j << ";\n";
            o << "        }\n";
        }
        o << cx.close_space();
    }
    o << "}\n";
    o << "extern \"C\" __global__ __launch_bounds__(256) void gen_apply_graph(GenArgs a, const T* __restrict__ p, T* __restrict__ Ap,\n"
         "        const T* __restrict__ dadd, const int* stop, ReduceSlot rs, int has_centred) {\n"
         "    if (stop && *stop) return;\n"
      << cx.top_coords() <<
         "    T dot = 0;\n";
    // 1-D vertex domains: the centred terms at this vertex too (after the edge loops,
    // whose registers are free by then), instead of a gen_apply pass that stores them
    // for this kernel to read back
    gs.graph_apply_centred = gs.has_centered && cx.nd == 1 && !cx.mspace;
    for (int sp : cx.uspaces) {
        o << open_vtx(sp);
        graph_gather(cx, o, true, sp);
        if (gs.graph_apply_centred) {
            std::string decl = "        T";
            for (int k : cx.unk)
                for (int ch = 0; ch < m.images[k].channels; ++ch)
                    decl += std::string(decl.size() > 9 ? "," : "") + " cacc" + std::to_string(uslot[k]) + "_" + std::to_string(ch) + " = 0";
            o << decl << ";\n        {\n        const long long lin = vtx;\n" << cx.coords_of(cx.nd);
            Body b(cx, o, cx.nd);
            centred_apply(cx, b, true, 0);
            o << "        }\n";
        }
        o << "        const bool act = (" << vflag << " & 1) != 0;\n";
        for (int k : cx.unk)
            for (int ch = 0; ch < m.images[k].channels && cx.in_space(k, sp); ++ch) {
                const std::string e = "a.uoff[" + std::to_string(uslot[k]) + "] + vtx * " +
                                      std::to_string(m.images[k].channels) + " + " + std::to_string(ch);
                const std::string sfx = std::to_string(uslot[k]) + "_" + std::to_string(ch);
                const std::string cen = gs.graph_apply_centred ? "cacc" + sfx : "(has_centred ? Ap[i] : (T)0)";
                o << "        { const long long i = " << e << "; const T pe = p[i];\n"
                  << "          const T o = act ? " << cen << " + acc" << sfx
                  << " + (dadd ? dadd[i] * pe : (T)0) : (T)0;\n"
                  << "          Ap[i] = o; dot += pe * o; }\n";
            }
        o << cx.close_space();
    }
    o << "    double v[1] = {(double)dot};\n    block_reduce_publish<1>(v, rs, blockIdx.x);\n}\n";
}

// ------------------------------------------------ block preconditioner: PCG kernels
// One thread per element of a block group; every group's channel count C and the
// positions of its channels in the unknown vector are literals here, so the C x C
// Cholesky, the inversion and the products unroll into registers (packed lower triangle:
// C (C + 1) / 2 values per thread). gen_blk_init factors M_e = B_e (+ diag CtC_e in LM),
// leaves M_e^-1 in place of B_e and forms z = M^-1 r, p = z, sum r.z; gen_blk_step2 /
// gen_blk_half2 are PCGStep2 / the residual reset's second half (stencil_driver.h:
// step2_kernel, half2_kernel; the same alpha, delta, r and q expressions) with
// z = M_e^-1 r written to its own vector; gen_blk_apply is z = M^-1 r alone.
// A pivot <= eps C max_i M_ii sends the element to the diagonal matrix of the scalar
// preconditioner's values (w: what gn_init_kernel / lm_init_kernel left in pre);
// excluded elements and those outside the owned range get M^-1 = 0.
void emit_block_pcg(const Ctx& cx, std::ostringstream& o) {
    if (!cx.blockpre) return;
    const GModel& m = cx.m;
    const std::vector<GBlockGroup>& groups = cx.groups;
    o << "#define OPT_TRI(i, j) ((i) * ((i) + 1) / 2 + (j))\n"
         "template <int C> __device__ __forceinline__ void opt_blk_invert(T (&m)[C * (C + 1) / 2], const T (&w)[C]) {\n"
         "    const T eps = sizeof(T) == 8 ? (T)2.220446049250313e-16 : (T)1.1920928955078125e-07;\n"
         "    T mx = m[0];\n"
         "#pragma unroll\n"
         "    for (int i = 1; i < C; ++i) mx = fmax(mx, m[OPT_TRI(i, i)]);\n"
         "    const T tol = eps * (T)C * mx;\n"
         "    bool ok = true;\n"
         "#pragma unroll\n"
         "    for (int j = 0; j < C; ++j) {   // Cholesky, L in place, its diagonal as 1 / L_jj\n"
         "        T d = m[OPT_TRI(j, j)];\n"
         "#pragma unroll\n"
         "        for (int k = 0; k < j; ++k) d -= m[OPT_TRI(j, k)] * m[OPT_TRI(j, k)];\n"
         "        ok = ok && d > tol;\n"
         "        const T is = (T)1 / sqrt(ok ? d : (T)1);\n"
         "        m[OPT_TRI(j, j)] = is;\n"
         "#pragma unroll\n"
         "        for (int i = j + 1; i < C; ++i) {\n"
         "            T v = m[OPT_TRI(i, j)];\n"
         "#pragma unroll\n"
         "            for (int k = 0; k < j; ++k) v -= m[OPT_TRI(i, k)] * m[OPT_TRI(j, k)];\n"
         "            m[OPT_TRI(i, j)] = v * is;\n"
         "        }\n"
         "    }\n"
         "#pragma unroll\n"
         "    for (int j = 0; j < C; ++j)   // L^-1 in place, column by column\n"
         "#pragma unroll\n"
         "        for (int i = j + 1; i < C; ++i) {\n"
         "            T v = m[OPT_TRI(i, j)] * m[OPT_TRI(j, j)];\n"
         "#pragma unroll\n"
         "            for (int k = j + 1; k < i; ++k) v += m[OPT_TRI(i, k)] * m[OPT_TRI(k, j)];\n"
         "            m[OPT_TRI(i, j)] = -v * m[OPT_TRI(i, i)];\n"
         "        }\n"
         "#pragma unroll\n"
         "    for (int i = 0; i < C; ++i)   // M^-1 = L^-T L^-1 in place, row by row\n"
         "#pragma unroll\n"
         "        for (int j = 0; j <= i; ++j) {\n"
         "            T v = 0;\n"
         "#pragma unroll\n"
         "            for (int k = i; k < C; ++k) v += m[OPT_TRI(k, i)] * m[OPT_TRI(k, j)];\n"
         "            m[OPT_TRI(i, j)] = v;\n"
         "        }\n"
         "    if (!ok) {\n"
         "#pragma unroll\n"
         "        for (int i = 0; i < C; ++i)\n"
         "#pragma unroll\n"
         "            for (int j = 0; j <= i; ++j) m[OPT_TRI(i, j)] = i == j ? w[i] : (T)0;\n"
         "    }\n"
         "}\n"
         "template <int C> __device__ __forceinline__ void opt_blk_mul(const T (&m)[C * (C + 1) / 2], const T (&x)[C], T (&y)[C]) {\n"
         "#pragma unroll\n"
         "    for (int i = 0; i < C; ++i) {\n"
         "        T v = 0;\n"
         "#pragma unroll\n"
         "        for (int j = 0; j < C; ++j) v += m[i >= j ? OPT_TRI(i, j) : OPT_TRI(j, i)] * x[j];\n"
         "        y[i] = v;\n"
         "    }\n"
         "}\n";
    // per group: its literals
    for (size_t g = 0; g < groups.size(); ++g) {
        const GBlockGroup& G = groups[g];
        const std::string sp = std::to_string(G.space);
        o << "struct OptGroup" << g << " {\n    static constexpr int C = " << G.C << ";\n"
          << "    static __device__ __forceinline__ long long n(const GenArgs& a) { return " << cx.blk_n((int)g) << "; }\n"
          << "    static __device__ __forceinline__ long long base(const GenArgs& a) { return " << cx.blk_base((int)g) << "; }\n"
          << "    static __device__ __forceinline__ bool act(const GenArgs& a, long long e) { return "
          << (cx.mspace ?"(a.flags[a.fbase[" + sp + "] + e] & 1) != 0" : "e >= a.own_lo && e < a.own_hi && (a.flags[e] & 1) != 0")
          << "; }\n"
          << "    static __device__ __forceinline__ void ix(const GenArgs& a, long long e, long long (&x)[" << G.C << "]) {\n";
        for (size_t q = 0; q < G.images.size(); ++q) {
            const int k = G.images[q], ch = m.images[k].channels;
            for (int c = 0; c < ch; ++c)
                o << "        x[" << G.first_row[q] + c << "] = a.uoff[" << cx.uslot[k] << "] + e * " << ch << " + " << c << ";\n";
        }
        o << "    }\n};\n";
    }
    o << "template <class G> __device__ __forceinline__ void opt_blk_load(const GenArgs& a, const T* blk, long long e, T (&m)[G::C * (G::C + 1) / 2]) {\n"
         "    const long long bN = G::n(a), bB = G::base(a);\n"
         "#pragma unroll\n"
         "    for (int j = 0; j < G::C * (G::C + 1) / 2; ++j) m[j] = blk[bB + (long long)j * bN + e];\n"
         "}\n"
         "template <class G> __device__ __forceinline__ T opt_blk_init_group(const GenArgs& a, const T* r, const T* pre, const T* ctc, T* blk, T* z, T* p, int lm) {\n"
         "    constexpr int C = G::C;\n"
         "    const long long bN = G::n(a), bB = G::base(a);\n"
         "    T acc = 0;\n"
         "    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < bN; e += (long long)gridDim.x * 256) {\n"
         "        long long x[C]; T m[C * (C + 1) / 2], rv[C], w[C], zv[C];\n"
         "        G::ix(a, e, x);\n"
         "        opt_blk_load<G>(a, blk, e, m);\n"
         "#pragma unroll\n"
         "        for (int i = 0; i < C; ++i) { rv[i] = r[x[i]]; w[i] = pre[x[i]]; if (lm) m[OPT_TRI(i, i)] += ctc[x[i]]; }\n"
         "        opt_blk_invert<C>(m, w);\n"
         "        const bool act = G::act(a, e);\n"
         "#pragma unroll\n"
         "        for (int j = 0; j < C * (C + 1) / 2; ++j) { m[j] = act ? m[j] : (T)0; blk[bB + (long long)j * bN + e] = m[j]; }\n"
         "        opt_blk_mul<C>(m, rv, zv);\n"
         "#pragma unroll\n"
         "        for (int i = 0; i < C; ++i) { z[x[i]] = zv[i]; p[x[i]] = zv[i]; acc += rv[i] * zv[i]; }\n"
         "    }\n"
         "    return acc;\n"
         "}\n"
         "template <class G> __device__ __forceinline__ void opt_blk_step2_group(const GenArgs& a, const T* p, const T* Ap, const T* blk, const T* b, T* r, T* delta, T* z,\n"
         "        T alpha, int first, int lm, int dl, T& acc_out, T& accq_out) {\n"
         "    constexpr int C = G::C;\n"
         "    const long long bN = G::n(a);\n"
         "    T acc = 0, accq = 0;\n"
         "    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < bN; e += (long long)gridDim.x * 256) {\n"
         "        long long x[C]; T m[C * (C + 1) / 2], rv[C], dv[C], zv[C];\n"
         "        G::ix(a, e, x);\n"
         "        opt_blk_load<G>(a, blk, e, m);\n"
         "#pragma unroll\n"
         "        for (int i = 0; i < C; ++i) {\n"
         "            const T rr = r[x[i]] - alpha * Ap[x[i]];\n"
         "            T d = 0;\n"
         "            if (dl) { d = first ? alpha * p[x[i]] : delta[x[i]] + alpha * p[x[i]]; delta[x[i]] = d; }\n"
         "            r[x[i]] = rr; rv[i] = rr; dv[i] = d;\n"
         "        }\n"
         "        opt_blk_mul<C>(m, rv, zv);\n"
         "#pragma unroll\n"
         "        for (int i = 0; i < C; ++i) {\n"
         "            z[x[i]] = zv[i];\n"
         "            acc += zv[i] * rv[i];\n"
         "            if (lm) accq += (T)0.5 * (dv[i] * (rv[i] + b[x[i]]));\n"
         "        }\n"
         "    }\n"
         "    acc_out += acc; accq_out += accq;\n"
         "}\n"
         "template <class G> __device__ __forceinline__ void opt_blk_half2_group(const GenArgs& a, const T* Adelta, const T* b, const T* blk, const T* delta, T* r, T* z, T& acc_out, T& accq_out) {\n"
         "    constexpr int C = G::C;\n"
         "    const long long bN = G::n(a);\n"
         "    T acc = 0, accq = 0;\n"
         "    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < bN; e += (long long)gridDim.x * 256) {\n"
         "        long long x[C]; T m[C * (C + 1) / 2], rv[C], zv[C];\n"
         "        G::ix(a, e, x);\n"
         "        opt_blk_load<G>(a, blk, e, m);\n"
         "#pragma unroll\n"
         "        for (int i = 0; i < C; ++i) { const T rr = b[x[i]] - Adelta[x[i]]; r[x[i]] = rr; rv[i] = rr; }\n"
         "        opt_blk_mul<C>(m, rv, zv);\n"
         "#pragma unroll\n"
         "        for (int i = 0; i < C; ++i) {\n"
         "            z[x[i]] = zv[i];\n"
         "            acc += zv[i] * rv[i];\n"
         "            accq += (T)0.5 * (delta[x[i]] * (rv[i] + b[x[i]]));\n"
         "        }\n"
         "    }\n"
         "    acc_out += acc; accq_out += accq;\n"
         "}\n"
         "template <class G> __device__ __forceinline__ void opt_blk_apply_group(const GenArgs& a, const T* blk, const T* rin, T* zout) {\n"
         "    constexpr int C = G::C;\n"
         "    const long long bN = G::n(a);\n"
         "    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < bN; e += (long long)gridDim.x * 256) {\n"
         "        long long x[C]; T m[C * (C + 1) / 2], rv[C], zv[C];\n"
         "        G::ix(a, e, x);\n"
         "        opt_blk_load<G>(a, blk, e, m);\n"
         "#pragma unroll\n"
         "        for (int i = 0; i < C; ++i) rv[i] = rin[x[i]];\n"
         "        opt_blk_mul<C>(m, rv, zv);\n"
         "#pragma unroll\n"
         "        for (int i = 0; i < C; ++i) zout[x[i]] = zv[i];\n"
         "    }\n"
         "}\n"
      << (cx.schur() ?
         "template <class G> __device__ __forceinline__ void opt_blk_clear_group(const GenArgs& a, T* z, T* p) {\n"
         "    constexpr int C = G::C;\n"
         "    const long long bN = G::n(a);\n"
         "    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < bN; e += (long long)gridDim.x * 256) {\n"
         "        long long x[C];\n"
         "        G::ix(a, e, x);\n"
         "#pragma unroll\n"
         "        for (int i = 0; i < C; ++i) { z[x[i]] = (T)0; p[x[i]] = (T)0; }\n"
         "    }\n"
         "}\n" : "") <<
         // LM inner-loop exit test on the launch's total q (stencil_driver.h zeta_test)
         "__device__ __forceinline__ void opt_blk_zeta(double q1, double* q0, int* zstop, int liter, float q_tol) {\n"
      // Eliminate: the loop's q is the reduced system's; q0[1] holds this step's constant
      // 1/2 b_e.M^-1 b_e (gen_schur_rhs), their sum the full model's value at (delta_r, delta_e*(delta_r))
      << (cx.schur() ? "    q1 += q0[1];\n" : "") <<
         "    const T Q1 = (T)q1, Q0 = (T)*q0;\n"
         "    const T zeta = (T)(liter + 1) * (Q1 - Q0) / Q1;\n"
         "    if (zeta < (T)q_tol) *zstop = 1;\n"
         "    else *q0 = (double)Q1;\n"
         "}\n";
    // Eliminate: during the PCG loop the eliminated group's r, z, p, Ap and delta are exactly
    // zero, so its elements take `elim` instead ("": nothing to do): gen_blk_init only clears
    // z and p (gen_schur_rhs has inverted the group's blocks already), the steps skip it
    auto each = [&](const std::string& call, const std::string& elim = "") {
        std::string s;
        for (size_t g = 0; g < groups.size(); ++g) {
            std::string c = (int)g == cx.elim_group ? elim : call;
            if (c.empty()) continue;
            c.replace(c.find("GROUP"), 5, "OptGroup" + std::to_string(g));
            s += "    " + c + "\n";
        }
        return s;
    };
    o << "extern \"C\" __global__ __launch_bounds__(256) void gen_blk_init(GenArgs a, const T* __restrict__ r, const T* __restrict__ pre,\n"
         "        const T* __restrict__ ctc, T* __restrict__ blk, T* __restrict__ z, T* __restrict__ p, int lm, ReduceSlot rs) {\n"
         "    T acc = 0;\n"
      << each("acc += opt_blk_init_group<GROUP>(a, r, pre, ctc, blk, z, p, lm);", "opt_blk_clear_group<GROUP>(a, z, p);")
      << "    double v[1] = {(double)acc};\n    block_reduce_publish<1>(v, rs, blockIdx.x);\n}\n";
    o << "extern \"C\" __global__ __launch_bounds__(256) void gen_blk_step2(GenArgs a, const T* __restrict__ p, const T* __restrict__ Ap,\n"
         "        const T* __restrict__ blk, const T* __restrict__ b, T* __restrict__ r, T* __restrict__ delta, T* __restrict__ z,\n"
         "        const double* __restrict__ sc, int i_num, int i_den, int first, int lm, int dl, const int* stop, ReduceSlot rs,\n"
         "        double* q0, int* zstop, int liter, float q_tol, int zon) {\n"
         "    if (stop && *stop) return;\n"
         "    const T alpha = (T)(sc[i_num] / sc[i_den]);\n"
         "    T acc = 0, accq = 0;\n"
      << each("opt_blk_step2_group<GROUP>(a, p, Ap, blk, b, r, delta, z, alpha, first, lm, dl, acc, accq);")
      << "    double v[2] = {(double)acc, (double)accq};\n"
         "    if (lm) {\n"
         "        double tot[2];\n"
         "        if (block_reduce_publish<2>(v, rs, blockIdx.x, tot) && zon) opt_blk_zeta(tot[1], q0, zstop, liter, q_tol);\n"
         "    } else {\n"
         "        double v1[1] = {v[0]};\n"
         "        block_reduce_publish<1>(v1, rs, blockIdx.x);\n"
         "    }\n}\n";
    o << "extern \"C\" __global__ __launch_bounds__(256) void gen_blk_half2(GenArgs a, const T* __restrict__ Adelta, const T* __restrict__ b,\n"
         "        const T* __restrict__ blk, const T* __restrict__ delta, T* __restrict__ r, T* __restrict__ z, const int* stop, ReduceSlot rs,\n"
         "        double* q0, int* zstop, int liter, float q_tol, int zon) {\n"
         "    if (stop && *stop) return;\n"
         "    T acc = 0, accq = 0;\n"
      << each("opt_blk_half2_group<GROUP>(a, Adelta, b, blk, delta, r, z, acc, accq);")
      << "    double v[2] = {(double)acc, (double)accq};\n"
         "    double tot[2];\n"
         "    if (block_reduce_publish<2>(v, rs, blockIdx.x, tot) && zon) opt_blk_zeta(tot[1], q0, zstop, liter, q_tol);\n}\n";
    o << "extern \"C\" __global__ __launch_bounds__(256) void gen_blk_apply(GenArgs a, const T* __restrict__ blk, const T* __restrict__ rin, T* __restrict__ zout) {\n"
      << each("opt_blk_apply_group<GROUP>(a, blk, rin, zout);", "opt_blk_apply_group<GROUP>(a, blk, rin, zout);") << "}\n";
}

}  // namespace gen
}  // namespace optamd
