// gen/codegen_strip.cpp — the register-strip kernels (gen_apply_strip, gen_jtf_strip,
// gen_cost_strip): each wave owns a column strip, one pixel per lane, and walks down a block
// of rows with every centred read served from per-array row windows held in registers.
#include <algorithm>
#include <cstdlib>
#include "codegen_ctx.h"

namespace optamd {
namespace gen {
namespace {

// The row windows of one strip kernel. While a Body emits the per-centre code, serve()
// answers its centred reads from window registers and records which rows (centre + dy) of
// which array each window must hold; afterwards the kernel emits, through this struct, the
// wave loop, the window declarations with their preload, and per row the roll and the
// one-row-ahead prefetch. The three kernels differ in the vector they read next to the
// images (vprefix, vec, nullable) and in the row their walk starts at (row0).
struct RowWindows {
    using Key = std::tuple<int, int, int>;   // (0 image / 1 the vector, image, channel)
    const Ctx& cx;
    const char* vprefix;   // name prefix of the vector's windows ("wp" / "wd"; images: "wi")
    const char* vec;       // the vector read at unknown accesses: "p" / "delta"
    bool nullable;         // it may be null (the cost): its loads are masked by it
    std::string row0;      // centre row of the walk's first iteration
    std::map<Key, std::pair<int, int>> win;   // rows each window must hold
    int rxlo = 0, rxhi = 0;                   // lane reach of the reads
    bool pairs = false, opq = false;          // open_waves: pair windows present, opt_at32<O>

    std::string wname(const Key& k, int dy) const {
        return std::string(std::get<0>(k) ? vprefix : "wi") + std::to_string(std::get<1>(k)) + "c" +
               std::to_string(std::get<2>(k)) + (dy < 0 ? "m" : "p") + std::to_string(std::abs(dy));
    }
    void serve(Body& b) {
        b.centred_reads([this](const Node& n, const char* vname) {
            const Key key(vname ? 1 : 0, n.i, n.ch);
            auto it = win.find(key);
            if (it == win.end()) win[key] = {n.off[1], n.off[1]};
            else it->second = {std::min(it->second.first, n.off[1]), std::max(it->second.second, n.off[1])};
            rxlo = std::min(rxlo, n.off[0]);
            rxhi = std::max(rxhi, n.off[0]);
            const std::string w = wname(key, n.off[1]);
            return n.off[0] == 0 ? w : "opt_sh(" + w + ", " + std::to_string(n.off[0]) + ")";
        });
    }
    int regs() const {
        int r = 0;
        for (auto& w : win) r += w.second.second - w.second.first + 2;   // + the prefetched row
        return r;
    }
    std::string base_of(const Key& k) const {
        const int i = std::get<1>(k);
        const GImage& im = cx.m.images[i];
        const std::string own = "((const " + std::string(elem_type(im.elem, im.tvalued)) + "*)a.img[" + std::to_string(i) + "])";
        if (!std::get<0>(k)) return own;
        const std::string v = std::string(vec) + " + a.uoff[" + std::to_string(cx.uslot[i]) + "]";
        // a null vector: the image itself stands in as a valid address
        return nullable ? "(" + std::string(vec) + " ? " + v + " : " + own + ")" : "(" + v + ")";
    }
    // the two channels of a 2-channel array whose windows span the same rows are
    // read as one 8 / 16-byte access (opt_ldm2)
    bool partner(const Key& k) const {
        const int i = std::get<1>(k);
        if (cx.m.images[i].channels != 2) return false;
        auto a0 = win.find(Key(std::get<0>(k), i, 0));
        auto a1 = win.find(Key(std::get<0>(k), i, 1));
        return a0 != win.end() && a1 != win.end() && a0->second == a1->second;
    }
    // The strip's prologue and its wave loop (emitted once pairs is known): the wave index
    // through readfirstlane in the kernels without pair windows (OPT_AMD_GEN_WIDU=2, the
    // default; 1 always, 0 never); 32-bit offsets opaque by the same rule (OPT_AMD_GEN_STRIP32)
    void open_waves(std::ostringstream& o, int nout, int loff) {
        for (auto& w : win) pairs = pairs || (std::get<2>(w.first) == 0 && partner(w.first));
        const Knobs& kn = cx.knobs;
        opq = kn.strip32 == 2 || (kn.strip32 == 4 && !pairs);   // opt_at32<O>
        o << "    const int lane = threadIdx.x & 63, z = 0; (void)z;\n"
             "    const int nsx = (W + " << nout - 1 << ") / " << nout << ", G = gridDim.x * 4;\n"
             "    const int RB = max(8, (int)(((long long)H * nsx + G - 1) / G)), nby = (H + RB - 1) / RB;\n";
        o << "    for (int wid = " << (kn.widu == 1 || (kn.widu == 2 && !pairs)
                                          ? "__builtin_amdgcn_readfirstlane((int)opt_xcd_block() * 4 + (threadIdx.x >> 6))"
                                          : "(int)opt_xcd_block() * 4 + (threadIdx.x >> 6)") << "; wid < nsx * nby; wid += G) {\n"
             "        const int x = (wid % nsx) * " << nout << " + lane - " << loff << ";\n"
             "        const int y0 = (wid / nsx) * RB, y1 = min(H, y0 + RB);\n"
             "        const bool xin = x >= 0 && x < W, xout = xin && lane >= " << loff << " && lane < " << loff + nout << ";\n";
    }
    // statement loading row yy of window k into `dst` (and of its partner channel)
    std::string load(const Key& k, const std::string& yy, int dy, const char* sfx) const {
        const bool s32 = cx.s32();
        const int i = std::get<1>(k), c = std::get<2>(k), ch = cx.m.images[i].channels;
        const std::string cond = "xin && " + yy + " >= 0 && " + yy + " < H" + (std::get<0>(k) && nullable ? " && " + std::string(vec) : "");
        const std::string pix = s32 ? "(unsigned)(" + yy + " * W + x) * " + std::to_string(ch) + "u"
                                        : "(long long)(" + yy + " * W + x) * " + std::to_string(ch);
        const std::string sf = s32 ? (opq ? "_32<true>(" : "_32<false>(") : "(";
        if (partner(k)) {
            if (c == 1) return std::string();
            const Key k1(std::get<0>(k), i, 1);
            return "opt_ldm2" + sf + base_of(k) + ", " + pix + ", " + cond + ", " + wname(k, dy) + sfx + ", " +
                   wname(k1, dy) + sfx + ");";
        }
        return wname(k, dy) + sfx + " = opt_ldm" + (s32 ? std::string(opq ? "32<true>(" : "32<false>(") : std::string("(")) + base_of(k) +
               ", " + pix + " + " + std::to_string(c) + ", " + cond + ");";
    }
    // each window's next top row is loaded one row ahead (<window>_n): its loads are
    // in flight during a whole row of residual arithmetic before they are consumed
    void declare_and_preload(std::ostringstream& o) const {
        for (auto& w : win) {
            o << "        T " << wname(w.first, w.second.second) << "_n = 0";
            for (int dy = w.second.first; dy <= w.second.second; ++dy) o << ", " << wname(w.first, dy) << " = 0";
            o << ";\n";
        }
        for (auto& w : win) {
            for (int dy = w.second.first + 1; dy <= w.second.second; ++dy) {
                const std::string st = load(w.first, "(" + row0 + " - 1 + " + std::to_string(dy) + ")", dy, "");
                if (!st.empty()) o << "        " << st << "\n";
            }
            const std::string st = load(w.first, "(" + row0 + " + " + std::to_string(w.second.second) + ")",
                                        w.second.second, "_n");
            if (!st.empty()) o << "        " << st << "\n";
        }
    }
    // inside the row loop (centre row y): every window one row down, the next top row's loads
    void roll_and_prefetch(std::ostringstream& o) const {
        for (auto& w : win) {
            for (int dy = w.second.first; dy < w.second.second; ++dy)
                o << "        " << wname(w.first, dy) << " = " << wname(w.first, dy + 1) << ";\n";
            o << "        " << wname(w.first, w.second.second) << " = " << wname(w.first, w.second.second) << "_n;\n";
        }
        for (auto& w : win) {
            const std::string st = load(w.first, "(y + " + std::to_string(w.second.second + 1) + ")", w.second.second, "_n");
            if (!st.empty()) o << "        " << st << "\n";
        }
    }
};

// no sampled reads in the residuals; none, and no slot reads, in the Exclude expression
bool strip_servable(const Ctx& cx, bool with_exclude) {
    const GModel& m = cx.m;
    bool ok = true;
    for (int ci : cx.cres)
        cx.P.visit(m.residuals[ci].expr, [&](int, const Node& n) { ok &= n.op != Op::Sample; });
    if (with_exclude && m.exclude >= 0)
        cx.P.visit(m.exclude, [&](int, const Node& n) { ok &= n.op != Op::Sample && !(n.op == Op::Read && n.slot >= 0); });
    return ok;
}

// Per centre: every centred residual's partials d<e> (the name of each entry's, returned)
// and jp<r> = its J p (apply) or its value (jtf), 0 where the centre is outside (qin).
std::vector<std::string> strip_residuals(Ctx& cx, Body& b, bool jtf) {
    const GModel& m = cx.m;
    Pool& P = cx.P;
    const std::vector<int>& cres = cx.cres;
    const std::vector<Entry>& ents = cx.ents;
    std::vector<std::string> dname(ents.size());
    for (size_t ci = 0; ci < cres.size(); ++ci) {
        // A residual Select(c1, Select(c2, e, 0), 0) has partials Select(c1, Select(c2,
        // de, 0), 0): its mask is evaluated once (m<ci>) and applied to Jp alone — each
        // partial's contribution d * Jp is then 0 with it — instead of a select per
        // partial; only when every partial is free of operations that can be non-finite
        // where the mask is off (division, sqrt, log, pow, exp; tan, sinh, cosh, asin,
        // acos, acosh, log10: out of domain or overflowing on whatever the masked data
        // holds), where 0 * d could be NaN. atan, tanh, asinh and atan2 are finite for
        // every finite input (and their partials hold a division anyway).
        std::vector<int> conds;
        std::vector<int> de(ents.size(), -1);
        bool factor = !jtf && cx.knobs.factor;
        if (factor) {
            int core = m.residuals[cres[ci]].expr;
            double z;
            while (P.at(core).op == Op::Select && P.is_const(P.at(core).d, &z) && z == 0.0) {
                conds.push_back(P.at(core).a);
                core = P.at(core).b;
            }
            factor = !conds.empty();
            for (size_t ei = 0; ei < ents.size() && factor; ++ei) {
                if (ents[ei].r != (int)ci || ents[ei].slot < 0) continue;
                int x = ents[ei].dnode;
                for (int c : conds) {
                    const Node& n = P.at(x);   // (the pool does not grow while n is live)
                    if (n.op == Op::Select && n.a == c && P.is_const(n.d, &z) && z == 0.0) x = n.b;
                    else { factor = false; break; }
                }
                P.visit(x, [&](int, const Node& n) {
                    factor = factor && n.op != Op::Div && n.op != Op::Sqrt && n.op != Op::Log &&
                             n.op != Op::Pow && n.op != Op::Exp && n.op != Op::Sample &&
                             n.op != Op::Tan && n.op != Op::Sinh && n.op != Op::Cosh &&
                             n.op != Op::Asin && n.op != Op::Acos && n.op != Op::Acosh &&
                             n.op != Op::Log10;
                });
                de[ei] = x;
            }
        }
        if (factor) {
            std::string mc = "qin";
            for (int c : conds) mc += " && " + b.cond(c);
            b.line("const bool m" + std::to_string(ci) + " = " + mc + ";");
            std::string fsum = "(T)0";
            for (size_t ei = 0; ei < ents.size(); ++ei) {
                if (ents[ei].r != (int)ci) continue;
                if (ents[ei].slot >= 0) {
                    dname[ei] = "d" + std::to_string(ei);
                    b.line("const T " + dname[ei] + " = " + b.v(de[ei]) + ";");
                } else {
                    double cv;
                    P.is_const(ents[ei].dnode, &cv);
                    dname[ei] = lit(cv);
                }
                fsum += " + " + dname[ei] + " * " + b.vec(ents[ei].u, "p");
            }
            b.line("const T jp" + std::to_string(ci) + " = m" + std::to_string(ci) + " ? " + fsum + " : (T)0;");
            // A partial that reads a known array (or a ComputedArray) may be non-finite
            // where the mask is off — NaN / Inf is a common "no data" value there — and
            // d * jp would then be NaN * 0. The reference's Select discards that branch,
            // so those partials keep the mask on their transpose contribution;
            // partials over unknowns, parameters and constants alone need none.
            for (size_t ei = 0; ei < ents.size(); ++ei) {
                if (ents[ei].r != (int)ci || ents[ei].slot < 0) continue;
                bool data = false;
                P.visit(de[ei], [&](int, const Node& n) {
                    data = data || (n.op == Op::Read && !(n.i >= 0 && n.i < (int)m.images.size() &&
                                                           m.images[n.i].unknown));
                });
                if (!data) continue;
                const std::string dm = "dm" + std::to_string(ei);
                b.line("const T " + dm + " = m" + std::to_string(ci) + " ? " + dname[ei] + " : (T)0;");
                dname[ei] = dm;
            }
            continue;
        }
        std::string sum = "(T)0";
        for (size_t ei = 0; ei < ents.size(); ++ei) {
            if (ents[ei].r != (int)ci) continue;
            const std::string dn = b.v(ents[ei].dnode);
            if (ents[ei].slot >= 0) {
                dname[ei] = "d" + std::to_string(ei);
                b.line("const T " + dname[ei] + " = qin ? " + dn + " : (T)0;");
            } else {
                double cv;
                P.is_const(ents[ei].dnode, &cv);
                dname[ei] = lit(cv);
            }
            if (!jtf) sum += " + " + dn + " * " + b.vec(ents[ei].u, "p");
        }
        if (jtf) b.line("const T jp" + std::to_string(ci) + " = qin ? " + b.v(m.residuals[cres[ci]].expr) + " : (T)0;");
        else b.line("const T jp" + std::to_string(ci) + " = qin ? " + sum + " : (T)0;");
    }
    return dname;
}

// ------------------------------------------------------------ gen_apply_strip
// J^T J p in registers: each wave owns a column strip (one pixel per lane, halo lanes
// at both ends) and walks down a block of rows. Every centred residual is evaluated
// ONCE per centre (as the tiled form), its reads served from per-array row windows
// (the rows centre + dy the residuals touch; a column offset dx is a DPP lane shift);
// each centre's contributions d(r, u) Jp_r are summed per output offset (u's offset),
// lane-shifted to the output column and added to rolling per-row accumulators; an
// output row is finished once the last centre row that reaches it has been evaluated.
// No LDS and no barriers: the hand-written image_warping / SFS applies work this way.
// Same instance set as createjtjcentered (o.t:2770-2830): centres outside the image
// contribute nothing (gen_apply_tiled's rule).
// gen_jtf_strip: the same walk for J^T F + diag(J^T J) + flags: each centre's residual
// values R_r and partials d(r, u) once, d R and d^2 accumulated per output offset; the
// output's Exclude is evaluated at the output row (shifted by miny). Same instance set.
void emit_scatter_strip(Ctx& cx, std::ostringstream& o, bool jtf) {
    GModel& m = cx.m;
    Pool& P = cx.P;
    GenSource& gs = cx.gs;
    const std::vector<int>&unk = cx.unk, &uslot = cx.uslot;
    const std::vector<Entry>& ents = cx.ents;
    const int minx = cx.minx, maxx = cx.maxx, miny = cx.miny, maxy = cx.maxy;
    const bool s32 = cx.s32();
    bool ok = strip_servable(cx, jtf);
    RowWindows rw{cx, "wp", "p", false, "(y0 - " + std::to_string(maxy) + ")"};
    std::ostringstream body, fin;
    {
        Body b(cx, body, cx.nd);
        b.use_pred(true);
        b.use_cache(false);
        rw.serve(b);
        const std::vector<std::string> dname = strip_residuals(cx, b, jtf);
        // contributions per output (image, channel, offset): one lane shift each
        // (jtf: jp holds the residual value; dg the squared partials)
        std::map<std::tuple<int, int, int, int>, std::pair<std::string, std::string>> grp;
        for (size_t ei = 0; ei < ents.size(); ++ei) {
            const Node n = P.at(ents[ei].u);
            auto& s = grp[std::make_tuple(n.i, n.ch, ents[ei].oy, ents[ei].ox)];
            s.first += (s.first.empty() ? "" : " + ") + dname[ei] + " * jp" + std::to_string(ents[ei].r);
            if (jtf) {
                // a constant partial still only counts where its centre is inside
                const std::string d = ents[ei].slot >= 0 ? dname[ei] : "(qin ? " + dname[ei] + " : (T)0)";
                s.second += (s.second.empty() ? "" : " + ") + d + " * " + d;
            }
        }
        for (auto& g : grp) {
            const int k = std::get<0>(g.first), c = std::get<1>(g.first), oy = std::get<2>(g.first),
                      ox = std::get<3>(g.first);
            const std::string sfx = std::to_string(uslot[k]) + "_" + std::to_string(c) + "_" + std::to_string(oy - miny);
            auto add = [&](const std::string& acc, const std::string& e) {
                b.line(acc + " += " + (ox == 0 ? "(" + e + ")" : "opt_sh(" + e + ", " + std::to_string(-ox) + ")") + ";");
            };
            add("ac" + sfx, g.second.first);
            if (jtf) add("dq" + sfx, g.second.second);
        }
        if (jtf) {
            // the output row's Exclude, read from the same windows
            Body bf(cx, fin, cx.nd);
            bf.use_pred(true);
            bf.use_cache(false);
            rw.serve(bf);
            const int sh[3] = {0, miny, 0};
            const std::string act = m.exclude >= 0 ? "(" + bf.v(cx.shifted(m.exclude, sh)) + " == (T)0)" : "true";
            bf.line("const bool act = " + act + ";");
        }
    }
    int regs = rw.regs();
    int nacc = 0;
    for (int k : unk) nacc += m.images[k].channels;
    regs += nacc * (maxy - miny + 1) * (jtf ? 2 : 1);
    const int loff = -rw.rxlo + maxx, nout = 64 + rw.rxlo - rw.rxhi - (maxx - minx);
    ok = ok && nout >= 16 && regs <= 96 * (cx.dbl ? 1 : 2) / 2;
    if (!ok) return;
    if (jtf) {
        gs.has_jtf_strip = true;
        gs.jtf_strip_cols = nout;
        o << "extern \"C\" __global__ __launch_bounds__(256) void gen_jtf_strip(GenArgs a, T* __restrict__ r, T* __restrict__ diag) {\n"
             "    OPT_COORDS\n";
    } else {
        gs.has_strip = true;
        gs.strip_cols = nout;
        o << "extern \"C\" __global__ __launch_bounds__(256) void gen_apply_strip(GenArgs a, const T* __restrict__ p, T* __restrict__ Ap,\n"
             "        const T* __restrict__ dadd, const int* stop, ReduceSlot rs, int finish) {\n"
             "    if (stop && *stop) return;\n"
             "    OPT_COORDS\n"
             "    T dot = 0;\n";
    }
    rw.open_waves(o, nout, loff);
    rw.declare_and_preload(o);
    for (int k : unk)
        for (int c = 0; c < m.images[k].channels; ++c)
            for (int j = 0; j <= maxy - miny; ++j) {
                o << "        T ac" << uslot[k] << "_" << c << "_" << j << " = 0;\n";
                if (jtf) o << "        T dq" << uslot[k] << "_" << c << "_" << j << " = 0;\n";
            }
    o << "        for (int y = " << rw.row0 << "; y < y1 - " << miny << "; ++y) {\n";
    rw.roll_and_prefetch(o);
    o << "        const bool qin = xin && y >= 0 && y < H;\n" << body.str();
    // output row y + miny has all its centres
    // (off32: the element index as a 32-bit byte offset from the array's base, opt_at32)
    const std::string ity = s32 ? "unsigned" : "long long";
    auto at = [&](const std::string& arr, const std::string& e) {
        return s32 ? std::string(rw.opq ? "opt_at32<true>(" : "opt_at32<false>(") + arr + ", " + e + ")" : arr + "[" + e + "]";
    };
    // An Exclude that reads at a column offset takes its value from a neighbouring lane (a DPP
    // shift), and a shift reads 0 from a lane that is switched off: inside the branch on xout
    // the halo lanes are, so the first output column of every strip but the leftmost saw its
    // left neighbour's mask as 0 and was never excluded. Such a test is evaluated before the
    // branch, by the whole wave (a test at the centre column stays where it was).
    const bool hoist = jtf && fin.str().find("opt_sh(") != std::string::npos;
    if (hoist) o << "        bool act_o;\n        {\n" << fin.str() << "        act_o = act;\n        }\n";
    o << "        const int yo = y + " << miny << ";\n"
         "        if (xout && yo >= y0 && yo < y1) {\n"
         "        const " << ity << " lin = (" << ity << ")yo * W + x;\n";
    if (hoist) o << "        const bool act = act_o;\n        " << at("a.flags", "lin") << " = act ? 1 : 0;\n";
    else if (jtf) o << fin.str() << "        " << at("a.flags", "lin") << " = act ? 1 : 0;\n";
    else o << "        const bool act = (" << at("a.flags", "lin") << " & 1) != 0;\n";
    for (int k : unk)
        for (int c = 0; c < m.images[k].channels; ++c) {
            const std::string el = "(" + ity + ")a.uoff[" + std::to_string(uslot[k]) + "] + lin * " +
                                   std::to_string(m.images[k].channels) + " + " + std::to_string(c);
            const std::string sfx = std::to_string(uslot[k]) + "_" + std::to_string(c) + "_0";
            if (jtf) {
                o << "        { const " << ity << " e = " << el << "; " << at("r", "e") << " = act ? -ac" << sfx
                  << " : (T)0; " << at("diag", "e") << " = dq" << sfx << "; }\n";
                continue;
            }
            // p at the output pixel: its row window when one holds row yo (same load)
            std::string pe = at("p", "e");
            auto wi = rw.win.find(RowWindows::Key(1, k, c));
            if (wi != rw.win.end() && wi->second.first <= miny && miny <= wi->second.second)
                pe = rw.wname(wi->first, miny);
            o << "        { const " << ity << " e = " << el << "; const T acc = ac" << sfx << ";\n"
                 "          if (finish) { const T pe = " << pe << "; const T o = act ? acc + (dadd ? " << at("dadd", "e")
              << " * pe : (T)0) : (T)0; " << at("Ap", "e") << " = o; dot += pe * o; }\n"
                 "          else " << at("Ap", "e") << " = acc; }\n";
        }
    o << "        }\n";
    for (int k : unk)
        for (int c = 0; c < m.images[k].channels; ++c)
            for (const char* an : {"ac", "dq"}) {
                if (!jtf && an[0] == 'd') continue;
                const std::string a0 = an + std::to_string(uslot[k]) + "_" + std::to_string(c) + "_";
                for (int j = 0; j < maxy - miny; ++j) o << "        " << a0 << j << " = " << a0 << j + 1 << ";\n";
                o << "        " << a0 << maxy - miny << " = 0;\n";
            }
    o << "        }\n"
         "    }\n";
    if (jtf) o << "}\n";
    else o << "    if (finish) { double v[1] = {(double)dot}; block_reduce_publish<1>(v, rs, blockIdx.x); }\n}\n";
}

// gen_cost_strip: cost / model cost (gen_cost's per-centre expression: excluded centres
// skipped, 1/2 sum r^2, or with delta the linearised residuals r + sum_u dr/du delta_u)
// with every read served from row windows (unknowns, knowns, delta) walked down a
// column strip, one pixel per lane and centre; no scatter, so no row lag.
void emit_cost_strip(Ctx& cx, std::ostringstream& o) {
    const GModel& m = cx.m;
    bool ok = !cx.cres.empty() && strip_servable(cx, true);
    for (auto& r : m.residuals) ok &= r.graph < 0;   // graph terms: gen_cost
    if (!ok) return;
    RowWindows rw{cx, "wd", "delta", true, "y0"};
    std::ostringstream body;
    {
        Body b(cx, body, cx.nd);
        b.use_pred(true);
        b.use_cache(false);
        rw.serve(b);
        b.line("bool on = xout && y >= y0 && y < y1;");
        if (m.exclude >= 0) b.line("on = on && " + b.v(m.exclude) + " == (T)0;");
        centred_cost_terms(cx, b, cx.cres);
        b.line("if (on) acc += (T)0.5 * s;");
    }
    const int loff = -rw.rxlo, nout = 64 + rw.rxlo - rw.rxhi;
    if (nout < 16 || rw.regs() > 96 * (cx.dbl ? 1 : 2) / 2) return;
    cx.gs.has_cost_strip = true;
    cx.gs.cost_strip_cols = nout;
    o << "extern \"C\" __global__ __launch_bounds__(256) void gen_cost_strip(GenArgs a, const T* __restrict__ delta, ReduceSlot rs) {\n"
         "    OPT_COORDS\n"
         "    T acc = 0;\n";
    rw.open_waves(o, nout, loff);
    rw.declare_and_preload(o);
    o << "        for (int y = y0; y < y1; ++y) {\n";
    rw.roll_and_prefetch(o);
    o << "        const bool qin = xin; (void)qin;\n" << body.str() << "        }\n    }\n"
         "    double v[1] = {(double)acc}; block_reduce_publish<1>(v, rs, blockIdx.x);\n}\n";
}

}  // namespace

void emit_strips(Ctx& cx, std::ostringstream& o) {
    emit_scatter_strip(cx, o, false);   // gen_apply_strip
    emit_scatter_strip(cx, o, true);    // gen_jtf_strip
    emit_cost_strip(cx, o);
}

}  // namespace gen
}  // namespace optamd
