// gen/codegen_schur.cpp — the Schur complement's kernels (Eliminate(X, ...)), emitted only for
// energies with the statement.
//
// With the unknowns split into retained (r) and eliminated (e) ones, the step's system
// A delta = b (A = J^T J, plus LM's diagonal) is [[B, E], [E^T, C]] with C block-diagonal: one
// block per element of the eliminated space (the front end checks that no residual reads two
// of them). PCG runs on S delta_r = b_r - E M^-1 b_e with S = B - E M^-1 E^T, M_e = C_e
// (+ diag CtC_e in LM); afterwards delta_e = M^-1 (b_e - E^T delta_r). All vectors keep the full
// layout; w (M^-1-sized products) and the stash of b_e are compact: the eliminated images'
// elements alone, image after image.
//   gen_schur_rhs    per eliminated element: M_e^-1 in place of the block (a pivot
//                    <= sqrt(eps) max_i M_ii holds the element fixed: M_e^-1 = 0), the stash
//                    of b_e, w = M^-1 b_e, r_e = b_e = 0 and the sum 1/2 b_e.M^-1 b_e
//   gen_schur_elim   per eliminated vertex: u = (E^T p_r) over its incidence lists (the vertex
//                    gather of gen_apply_graph, p read at the retained images only), then
//                    out = M^-1 (rhs - u), or -M^-1 u without rhs
//   gen_schur_apply  per retained vertex: the gather with the eliminated images read from w
//                    and the others from p (a literal of each read), the retained spaces'
//                    centred terms and dadd p: Ap_r = B p_r + E w; 0 into Ap_e; p.Ap
// One lane per vertex, fixed summation order, no atomics (as the graph gathers).
#include "codegen_ctx.h"

namespace optamd {
namespace gen {

void emit_schur(Ctx& cx, std::ostringstream& o) {
    if (!cx.schur()) return;
    GModel& m = cx.m;
    const std::vector<int>& uslot = cx.uslot;
    const int eg = cx.elim_group, es = cx.elim_space();
    const GBlockGroup& G = cx.groups[eg];
    const std::string Gs = "OptGroup" + std::to_string(eg), ess = std::to_string(es);
    cx.gs.has_schur = true;
    // first element of an eliminated image inside the compact vectors
    auto woff = [&](int image) {
        std::string s = "0LL";
        for (int k : G.images) {
            if (k == image) break;
            s += " + " + std::to_string(m.images[k].channels) + "LL * a.snpix[" + ess + "]";
        }
        return s;
    };
    cx.vec_base = [&](int image, const char* vname) {
        if (std::string(vname) == "w") return "w + (" + woff(image) + ")";
        return std::string(vname) + " + a.uoff[" + std::to_string(uslot[image]) + "]";
    };
    auto open_vtx = [&](int sp) {
        const std::string s = std::to_string(sp);
        return "    {\n    const int W = a.sdims[" + s + "][0], H = a.sdims[" + s + "][1], D = a.sdims[" + s + "][2]; (void)W; (void)H; (void)D;\n"
               "    const long long fb = a.fbase[" + s + "]; (void)fb;\n"
               "    for (long long vtx = opt_xcd_block() * 256 + threadIdx.x; vtx < a.snpix[" + s + "]; vtx += (long long)gridDim.x * 256) {\n";
    };

    o << "struct OptElim {   // rows of the eliminated group inside the compact vectors\n"
         "    static __device__ __forceinline__ void lx(const GenArgs& a, long long e, long long (&x)[" << G.C << "]) {\n";
    for (size_t q = 0; q < G.images.size(); ++q) {
        const int k = G.images[q], ch = m.images[k].channels;
        for (int c = 0; c < ch; ++c)
            o << "        x[" << G.first_row[q] + c << "] = " << woff(k) << " + e * " << ch << " + " << c << ";\n";
    }
    o << "    }\n};\n";
    // Cholesky as opt_blk_invert, with the eliminated blocks' rule: M^-1 multiplies rounding
    // error by 1 / (pivot ratio), so a pivot <= sqrt(eps) max_i M_ii gives M^-1 = 0 (the element
    // stays where it is for this step; S is then that of the problem without its columns)
    o << "template <int C> __device__ __forceinline__ void opt_schur_invert(T (&m)[C * (C + 1) / 2]) {\n"
         "    const T seps = sizeof(T) == 8 ? (T)1.4901161193847656e-08 : (T)3.4526698300124393e-04;\n"
         "    T mx = m[0];\n"
         "#pragma unroll\n"
         "    for (int i = 1; i < C; ++i) mx = fmax(mx, m[OPT_TRI(i, i)]);\n"
         "    const T tol = seps * mx;\n"
         "    bool ok = true;\n"
         "#pragma unroll\n"
         "    for (int j = 0; j < C; ++j) {\n"
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
         "    for (int j = 0; j < C; ++j)\n"
         "#pragma unroll\n"
         "        for (int i = j + 1; i < C; ++i) {\n"
         "            T v = m[OPT_TRI(i, j)] * m[OPT_TRI(j, j)];\n"
         "#pragma unroll\n"
         "            for (int k = j + 1; k < i; ++k) v += m[OPT_TRI(i, k)] * m[OPT_TRI(k, j)];\n"
         "            m[OPT_TRI(i, j)] = -v * m[OPT_TRI(i, i)];\n"
         "        }\n"
         "#pragma unroll\n"
         "    for (int i = 0; i < C; ++i)\n"
         "#pragma unroll\n"
         "        for (int j = 0; j <= i; ++j) {\n"
         "            T v = 0;\n"
         "#pragma unroll\n"
         "            for (int k = i; k < C; ++k) v += m[OPT_TRI(k, i)] * m[OPT_TRI(k, j)];\n"
         "            m[OPT_TRI(i, j)] = ok ? v : (T)0;\n"
         "        }\n"
         "}\n";

    o << "extern \"C\" __global__ __launch_bounds__(256) void gen_schur_rhs(GenArgs a, T* __restrict__ blk, const T* __restrict__ ctc,\n"
         "        T* __restrict__ r, T* __restrict__ b, T* __restrict__ be, T* __restrict__ w, int lm, ReduceSlot rs) {\n"
         "    typedef " << Gs << " G;\n"
         "    constexpr int C = G::C;\n"
         "    const long long bN = G::n(a), bB = G::base(a);\n"
         "    T acc = 0;\n"
         "    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < bN; e += (long long)gridDim.x * 256) {\n"
         "        long long x[C], l[C]; T m[C * (C + 1) / 2], rv[C], wv[C];\n"
         "        G::ix(a, e, x);\n"
         "        OptElim::lx(a, e, l);\n"
         "        opt_blk_load<G>(a, blk, e, m);\n"
         "#pragma unroll\n"
         "        for (int i = 0; i < C; ++i) { rv[i] = r[x[i]]; if (lm) m[OPT_TRI(i, i)] += ctc[x[i]]; }\n"
         "        opt_schur_invert<C>(m);\n"
         "        const bool act = G::act(a, e);\n"
         "#pragma unroll\n"
         "        for (int j = 0; j < C * (C + 1) / 2; ++j) { m[j] = act ? m[j] : (T)0; blk[bB + (long long)j * bN + e] = m[j]; }\n"
         "        opt_blk_mul<C>(m, rv, wv);\n"
         "#pragma unroll\n"
         "        for (int i = 0; i < C; ++i) {\n"
         "            be[l[i]] = rv[i]; w[l[i]] = wv[i]; r[x[i]] = (T)0;\n"
         "            if (lm) b[x[i]] = (T)0;\n"
         "            acc += (T)0.5 * (rv[i] * wv[i]);\n"
         "        }\n"
         "    }\n"
         "    double v[1] = {(double)acc};\n    block_reduce_publish<1>(v, rs, blockIdx.x);\n}\n";

    // (p and out may be the same vector — the back-substitution reads delta's retained images
    // and writes its eliminated ones — so neither is __restrict__)
    o << "extern \"C\" __global__ __launch_bounds__(256) void gen_schur_elim(GenArgs a, const T* __restrict__ blk, const T* p,\n"
         "        const T* __restrict__ rhs, T* out, int out_full) {\n"
         "    typedef " << Gs << " G;\n"
         "    constexpr int C = G::C;\n";
    o << open_vtx(es);
    graph_gather(cx, o, true, es, 1);
    o << "        long long x[C], l[C]; T m[C * (C + 1) / 2], u[C], ov[C];\n"
         "        G::ix(a, vtx, x);\n"
         "        OptElim::lx(a, vtx, l);\n"
         "        opt_blk_load<G>(a, blk, vtx, m);\n";
    for (size_t q = 0; q < G.images.size(); ++q)
        for (int c = 0; c < m.images[G.images[q]].channels; ++c) {
            const int row = G.first_row[q] + c;
            const std::string acc = "acc" + std::to_string(uslot[G.images[q]]) + "_" + std::to_string(c);
            o << "        u[" << row << "] = rhs ? rhs[l[" << row << "]] - " << acc << " : -" << acc << ";\n";
        }
    o << "        opt_blk_mul<C>(m, u, ov);\n"
         "#pragma unroll\n"
         "        for (int i = 0; i < C; ++i) out[out_full ? x[i] : l[i]] = ov[i];\n"
      << cx.close_space() << "}\n";

    o << "extern \"C\" __global__ __launch_bounds__(256) void gen_schur_apply(GenArgs a, const T* __restrict__ p, const T* __restrict__ w,\n"
         "        T* __restrict__ Ap, const T* __restrict__ dadd, const int* stop, ReduceSlot rs) {\n"
         "    if (stop && *stop) return;\n"
         "    T dot = 0;\n";
    for (int sp : cx.uspaces) {
        if (sp == es) continue;
        o << open_vtx(sp);
        graph_gather(cx, o, true, sp, 2);
        bool centred = false;
        for (auto& r : m.residuals) centred |= r.graph < 0 && r.space == sp;
        if (centred) {
            std::string decl = "        T";
            for (int k : cx.unk)
                for (int ch = 0; ch < m.images[k].channels && cx.in_space(k, sp); ++ch)
                    decl += std::string(decl.size() > 9 ? "," : "") + " cacc" + std::to_string(uslot[k]) + "_" + std::to_string(ch) + " = 0";
            o << decl << ";\n        {\n        const long long lin = vtx;\n" << cx.coords_of(cx.nd_of(sp));
            Body b(cx, o, cx.nd_of(sp));
            centred_apply(cx, b, true, sp);
            o << "        }\n";
        }
        o << "        const bool act = (a.flags[fb + vtx] & 1) != 0;\n";
        for (int k : cx.unk)
            for (int ch = 0; ch < m.images[k].channels && cx.in_space(k, sp); ++ch) {
                const std::string e = "a.uoff[" + std::to_string(uslot[k]) + "] + vtx * " +
                                      std::to_string(m.images[k].channels) + " + " + std::to_string(ch);
                const std::string sfx = std::to_string(uslot[k]) + "_" + std::to_string(ch);
                o << "        { const long long i = " << e << "; const T pe = p[i];\n"
                  << "          const T o = act ? " << (centred ? "cacc" + sfx : std::string("(T)0")) << " + acc" << sfx
                  << " + (dadd ? dadd[i] * pe : (T)0) : (T)0;\n"
                  << "          Ap[i] = o; dot += pe * o; }\n";
            }
        o << cx.close_space();
    }
    o << "    {\n    constexpr int C = " << Gs << "::C;\n"
         "    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < " << Gs << "::n(a); e += (long long)gridDim.x * 256) {\n"
         "        long long x[C];\n"
         "        " << Gs << "::ix(a, e, x);\n"
         "#pragma unroll\n"
         "        for (int i = 0; i < C; ++i) Ap[x[i]] = (T)0;\n"
         "    }\n    }\n"
         "    double v[1] = {(double)dot};\n    block_reduce_publish<1>(v, rs, blockIdx.x);\n}\n";
    cx.vec_base = nullptr;
}

}  // namespace gen
}  // namespace optamd
