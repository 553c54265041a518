// gen/codegen.cpp — HIP kernels for a lowered energy (gen/model.h), compiled at plan
// time with hiprtc (generic.hip).
//
// Kernel semantics follow the reference's derived functions (API/src/o.t):
//   gen_jtf        createjtfcentered (:2870-2913): for every unknown x of a pixel, the sum
//                  over the centred residual instances containing x of dr/dx * r and
//                  (dr/dx)^2 (the instances are the residual templates shifted by the
//                  inverse of each support offset, residualsincludingX00 :2723-2733);
//                  writes r = -J^T F (0 on excluded unknowns), diag, and the exclude flags
//   gen_apply      createjtjcentered (:2770-2830): sum over the same instances of
//                  dr/dx * sum_u dr/du p(u); with `finish`, masks excluded unknowns, adds
//                  the LM diagonal and reduces p.Ap (PCGStep1, solverGPUGaussNewton.t:607-632)
//   gen_cost       createcost / createmodelcost (:3119-3129, :2915-2966): 1/2 sum r^2 (or
//                  (r + J delta)^2) over non-excluded centres, plus every graph edge
//   gen_*_graph    createjtfgraph / createjtjgraph (:2969-2994, :2833-2867): per edge,
//                  scattered to the edge's vertices with atomics as the reference does
//                  (Image:atomicAddChannel, backend_cuda.t:751-759)
// Reads outside the index space are zero (Image:get, o.t:856-862); centred residuals are
// wrapped in their bounding-box test at classification time.
//
// generate() keeps all its state in one Ctx (codegen_ctx.h) and is re-entrant. The Body
// expression emitter is in codegen_body.cpp, the register strips in codegen_strip.cpp, the
// graph gathers and the block preconditioner's PCG kernels in codegen_graph.cpp, the Schur
// complement's kernels (Eliminate) in codegen_schur.cpp.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include "codegen_ctx.h"
#include "reduce_dev_src.h"

#define OPTAMD_STR2(...) #__VA_ARGS__
#define OPTAMD_STR(x) OPTAMD_STR2(x)

namespace optamd {
namespace gen {

static Knobs read_knobs() {
    Knobs k;
    auto num = [](const char* name, int dflt) {
        const char* v = getenv(name);
        return v ? atoi(v) : dflt;
    };
    k.strip32 = num("OPT_AMD_GEN_STRIP32", 4);
    k.widu = num("OPT_AMD_GEN_WIDU", 2);
    k.factor = num("OPT_AMD_GEN_FACTOR", 1) != 0;
    k.prefetch_nb = num("OPT_AMD_GEN_NB_PREFETCH", 1) != 0;
    k.edge_unroll = num("OPT_AMD_GEN_EDGE_UNROLL", 4);
    k.pred = num("OPT_AMD_GEN_PRED", 1) != 0;
    k.graph_cache = num("OPT_AMD_GEN_GRAPH_CACHE", 1) != 0;
    return k;
}

Analysis::Analysis(const GModel& m)
    : nd(m.unknown_dims()), unk(m.unknown_images()), uslot(m.images.size(), -1), mspace(m.multi()),
      uspaces(mspace ? m.unknown_spaces() : std::vector<int>{0}), blockpre(m.block_preconditioner),
      groups(blockpre ? m.block_groups() : std::vector<GBlockGroup>{}), elim_group(-1) {
    for (size_t k = 0; k < unk.size(); ++k) uslot[unk[k]] = (int)k;
    for (size_t g = 0; g < groups.size() && m.schur(); ++g)
        if (groups[g].space == m.elim_space) elim_group = (int)g;
    for (size_t ri = 0; ri < m.residuals.size(); ++ri) {
        const GResidual& r = m.residuals[ri];
        if (r.graph >= 0) continue;
        for (int u : r.unknowns) {
            const Node n = m.pool.at(u);
            Instance I{(int)ri, {-n.off[0], -n.off[1], -n.off[2]}};
            inst[{n.i, n.ch}].push_back({I, u});
        }
    }
}

// memory pixel index -> coordinates; 2-D energies may hold a row slab whose memory row 0
// is global row a.ymem0 (coordinates, bounds and Index(1) are global)
// (32-bit unsigned divisions: the pixel index fits an int, as `li` assumes; a 64-bit
// division is a ~100-instruction sequence per pixel)
const char* Ctx::coords_of(int ndim) const {
    return ndim == 2 ? "        const unsigned ul = (unsigned)lin, uq = ul / (unsigned)W;\n"
                       "        const int x = (int)(ul - uq * (unsigned)W); const int y = (int)uq + a.ymem0; const int z = 0;\n"
                       "        const int li = (int)lin; (void)x; (void)y; (void)z; (void)li;\n"
                     : "        const unsigned ul = (unsigned)lin, uq = ul / (unsigned)W, uz = uq / (unsigned)H;\n"
                       "        const int x = (int)(ul - uq * (unsigned)W); const int y = (int)(uq - uz * (unsigned)H); const int z = (int)uz;\n"
                       "        const int li = (int)lin; (void)x; (void)y; (void)z; (void)li;\n";
}
std::string Ctx::open_space(int sp) const {
    if (mspace && (sp < 0 || sp >= (int)m.spaces.size())) {
        fprintf(stderr, "[opt_amd] codegen: kernel loop over an unknown index space %d\n", sp);
        abort();
    }
    if (!mspace)
        return std::string("    for (long long lin = a.own_lo + (long long)blockIdx.x * 256 + threadIdx.x; lin < a.own_hi; lin += (long long)gridDim.x * 256) {\n") +
               coords_of(nd);
    const std::string s = std::to_string(sp);
    return "    {\n    const int W = a.sdims[" + s + "][0], H = a.sdims[" + s + "][1], D = a.sdims[" + s + "][2]; (void)H; (void)D;\n"
           "    const long long fb = a.fbase[" + s + "]; (void)fb;\n"
           "    for (long long lin = (long long)blockIdx.x * 256 + threadIdx.x; lin < a.snpix[" + s + "]; lin += (long long)gridDim.x * 256) {\n" +
           coords_of(nd_of(sp));
}
int Ctx::group_of(int sp) const {
    for (size_t g = 0; g < groups.size(); ++g)
        if (!mspace || groups[g].space == sp) return (int)g;
    return -1;
}
std::string Ctx::blk_n(int g) const { return mspace ? "a.snpix[" + std::to_string(groups[g].space) + "]" : std::string("a.npix"); }
std::string Ctx::blk_base(int g) const {
    std::string s = "0LL";
    for (int q = 0; q < g; ++q) s += " + " + std::to_string(groups[q].entries()) + "LL * " + blk_n(q);
    return s;
}
int Ctx::blk_row(int g, int image, int ch) const {
    for (size_t q = 0; q < groups[g].images.size(); ++q)
        if (groups[g].images[q] == image) return groups[g].first_row[q] + ch;
    return -1;
}
// the one-space element loop with its coordinates, as the cache builders open it
static std::string open_owned(const Ctx& cx) {
    return std::string("    OPT_COORDS\n"
                       "    for (long long lin = a.own_lo + (long long)blockIdx.x * 256 + threadIdx.x; lin < a.own_hi; lin += (long long)gridDim.x * 256) {\n") +
           cx.coords_of(cx.nd);
}

void emit_prelude(const Ctx& cx, std::ostringstream& o) {
    const bool dbl = cx.dbl;
    const GModel& m = cx.m;
    o << "// generated by opt_amd's energy front end (gen/codegen.cpp)\n";
    o << "typedef " << (dbl ? "double" : "float") << " T;\n";
    o << "typedef T OptV4 __attribute__((ext_vector_type(4)));\n";
    o << "struct GenArgs { " << OPTAMD_STR(OPTAMD_GENARGS_FIELDS)
      << (m.multi() || !m.loss.empty() ? " " OPTAMD_STR(OPTAMD_GENARGS_SPACES) : "")
      << (!m.loss.empty() ? " " OPTAMD_STR(OPTAMD_GENARGS_LOSS) : "") << " };\n";
    o << kReduceDevSrc << "\n";
    o << "#define OPT_COORDS const int W = a.dims[0], H = a.dims[1], D = a.dims[2]; (void)D;\n";
    o << "__device__ __forceinline__ void opt_sincos(float x, float* s, float* c) { sincosf(x, s, c); }\n"
         "__device__ __forceinline__ void opt_sincos(double x, double* s, double* c) { sincos(x, s, c); }\n";
    // whole-wave DPP lane shifts (wave_shl:1 / wave_shr:1): opt_sh(v, d) is v of lane l + d
    // (0 past the wave's ends); d is a literal at every use, so the loops unroll away
    // (bound_ctrl: the hardware shifts 0 into the end lane, no register set to 0 first).
    // An energy that reads further than one column away chains shifts (|d| > 1), and its
    // loops carry `#pragma unroll`: left to the optimizer's own unroller after inlining, a
    // kernel with several chained shifts (gen_jtf_strip of an energy with offsets (2,-1) and
    // (-2,3), in float) crashed the compiler inside hiprtcCompileProgram. Radius-1 energies
    // keep the plain loops, and with them their source byte for byte.
    bool wide = false;
    {
        std::vector<int> roots;
        for (auto& r : m.residuals) roots.push_back(r.expr);
        for (auto& x : m.excludes) roots.push_back(x.second);
        for (int e : roots)
            m.pool.visit(e, [&](int, const Node& n) { wide = wide || (n.op == Op::Read && n.slot < 0 && std::abs(n.off[0]) > 1); });
    }
    o << "__device__ __forceinline__ float opt_lr(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130, 0xf, 0xf, true)); }\n"
         "__device__ __forceinline__ float opt_ll(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, true)); }\n"
         "__device__ __forceinline__ double opt_dd(double v, bool r) {\n"
         "    const long long b = __double_as_longlong(v);\n"
         "    const int lo = r ? __builtin_amdgcn_update_dpp(0, (int)b, 0x130, 0xf, 0xf, true) : __builtin_amdgcn_update_dpp(0, (int)b, 0x138, 0xf, 0xf, true);\n"
         "    const int hi = r ? __builtin_amdgcn_update_dpp(0, (int)(b >> 32), 0x130, 0xf, 0xf, true) : __builtin_amdgcn_update_dpp(0, (int)(b >> 32), 0x138, 0xf, 0xf, true);\n"
         "    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);\n}\n"
         "__device__ __forceinline__ double opt_lr(double v) { return opt_dd(v, true); }\n"
         "__device__ __forceinline__ double opt_ll(double v) { return opt_dd(v, false); }\n";
    if (wide)
        o << "__device__ __forceinline__ T opt_sh(T v, int d) {\n"
             "    _Pragma(\"unroll\") for (; d > 0; --d) v = opt_lr(v);\n"
             "    _Pragma(\"unroll\") for (; d < 0; ++d) v = opt_ll(v);\n"
             "    return v;\n}\n";
    else
        o << "__device__ __forceinline__ T opt_sh(T v, int d) { for (; d > 0; --d) v = opt_lr(v); for (; d < 0; ++d) v = opt_ll(v); return v; }\n";
    // masked read without a branch: the load always issues (at element 0 of the array when
    // the access is outside), the value is selected afterwards
    // XCD-contiguous block order for the graph kernels and the register strips: the
    // hardware deals blocks to the 8 XCDs round robin, so with blockIdx order a vertex's
    // mesh neighbours (v +- 1, v +- a row) are gathered on several XCDs and cached in each
    // one's L2; with this order each XCD walks one contiguous eighth of the vertices (of
    // each grid-stride pass), and neighbouring strips, which share their halo columns, run
    // on the same XCD (generated image_warping / shape_from_shading GN / LM steps 6.91-6.92 ->
    // 6.86 / 3.87-3.89 -> 3.84-3.85 ms, same box; the grid-stride centred kernels gained
    // nothing, poisson's lost: they keep blockIdx order)
    o << "__device__ __forceinline__ long long opt_xcd_block() {\n"
         "    const int nb = gridDim.x, b = blockIdx.x, q = nb / 8, r = nb % 8, x = b % 8;\n"
         "    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + b / 8;\n}\n";
    // element v * stride + c of b, addressed as b + a 32-bit byte offset to element v's
    // record (generate's off32) + c: the channel stays a constant offset of the same
    // address, so a record's channels merge into one multi-dword load (a channel inside
    // the 32-bit sum cannot: the compiler must allow for its wrap-around)
    o << "template <typename E> __device__ __forceinline__ E opt_g32(const E* b, int v, unsigned stride, unsigned c) {\n"
         "    return ((const E*)((const char*)b + (unsigned)v * (stride * (unsigned)sizeof(E))))[c];\n}\n";
    // the same reads and element access through a 32-bit byte offset from a uniform base
    // (generate's off32: every array below 2 GiB): global_load / global_store with an SGPR
    // base and one VGPR offset, no 64-bit address arithmetic per access
    // O: the byte offset passes through an empty asm (opt_o32). Left visible, the compiler
    // shares one 64-bit extension of it between arrays and adds each base in 64 bits per
    // access; kept opaque, every access takes the SGPR-base form — which measured faster for
    // kernels whose windows are all single-channel (generated shape_from_shading 161 ->
    // 150 us) and slower where two-channel pair reads share the offsets (image_warping 192 ->
    // 205 us), so the strip kernels choose per kernel (OPT_AMD_GEN_STRIP32)
    o << "__device__ __forceinline__ unsigned opt_o32(unsigned o) { asm(\"\" : \"+v\"(o)); return o; }\n"
         "template <bool O, typename E> __device__ __forceinline__ const E& opt_at32(const E* b, unsigned i) {\n"
         "    const unsigned o = i * (unsigned)sizeof(E); return *(const E*)((const char*)b + (O ? opt_o32(o) : o));\n}\n"
         "template <bool O, typename E> __device__ __forceinline__ E& opt_at32(E* b, unsigned i) {\n"
         "    const unsigned o = i * (unsigned)sizeof(E); return *(E*)((char*)b + (O ? opt_o32(o) : o));\n}\n"
         "template <bool O, typename E> __device__ __forceinline__ T opt_ldm32(const E* b, unsigned i, bool c) {\n"
         "    const E v = opt_at32<O>(b, c ? i : 0u); return c ? (T)v : (T)0;\n}\n"
         "template <bool O, typename E> __device__ __forceinline__ void opt_ldm2_32(const E* b, unsigned i, bool c, T& v0, T& v1) {\n"
         "    const unsigned j = c ? i : 0u;\n"
         "    E x, y;\n"
         "    if ((((unsigned long long)b) & (2 * sizeof(E) - 1)) == 0) {\n"
         "        struct alignas(2 * sizeof(E)) P2 { E x, y; };\n"
         "        const unsigned o = j * (unsigned)sizeof(E);\n"
         "        const P2 v = *(const P2*)((const char*)b + (O ? opt_o32(o) : o)); x = v.x; y = v.y;\n"
         "    } else { x = opt_at32<O>(b, j); y = opt_at32<O>(b, j + 1); }\n"
         "    v0 = c ? (T)x : (T)0; v1 = c ? (T)y : (T)0;\n}\n";
    o << "template <typename E> __device__ __forceinline__ T opt_ldm(const E* b, long long i, bool c) {\n"
         "    const E v = b[c ? i : 0]; return c ? (T)v : (T)0;\n}\n"
         // both channels of a 2-channel element (i = its first channel) in one access when
         // the array is aligned for it (a uniform branch), else two
         "template <typename E> __device__ __forceinline__ void opt_ldm2(const E* b, long long i, bool c, T& v0, T& v1) {\n"
         "    const long long j = c ? i : 0;\n"
         "    E x, y;\n"
         "    if ((((unsigned long long)b) & (2 * sizeof(E) - 1)) == 0) {\n"
         "        struct alignas(2 * sizeof(E)) P2 { E x, y; };\n"
         "        const P2 v = *reinterpret_cast<const P2*>(b + j); x = v.x; y = v.y;\n"
         "    } else { x = b[j]; y = b[j + 1]; }\n"
         "    v0 = c ? (T)x : (T)0; v1 = c ? (T)y : (T)0;\n}\n";
    // Image:get / Image:sample (o.t:856-876): floor / ceil taps, zero outside, lerps in T
    o << "template <typename E> __device__ __forceinline__ T opt_tap(const E* im, int nch, int c, int x, int y, int W, int H) {\n"
         "    return (x >= 0 && x < W && y >= 0 && y < H) ? (T)im[((long long)y * W + x) * nch + c] : (T)0;\n}\n"
         "template <typename E> __device__ __forceinline__ T opt_sample(const E* im, int nch, int c, T x, T y, int W, int H) {\n"
         "    const int x0 = (int)floor(x), x1 = (int)ceil(x), y0 = (int)floor(y), y1 = (int)ceil(y);\n"
         "    const T xn = x - (T)x0, yn = y - (T)y0;\n"
         "    const T u = ((T)1 - xn) * opt_tap(im, nch, c, x0, y0, W, H) + xn * opt_tap(im, nch, c, x1, y0, W, H);\n"
         "    const T b = ((T)1 - xn) * opt_tap(im, nch, c, x0, y1, W, H) + xn * opt_tap(im, nch, c, x1, y1, W, H);\n"
         "    return ((T)1 - yn) * u + yn * b;\n}\n";
}

// --------------------------------------------- gen_precompute_<k> (ComputedArrays)
// One kernel per ComputedArray, launched in declaration order (a later one may read an
// earlier one at an offset): the values and the non-constant gradient images
// (createprecomputed, o.t:3131-3153).
void emit_precompute(Ctx& cx, std::ostringstream& o) {
    const GModel& m = cx.m;
    for (size_t k = 0; k < m.computed.size(); ++k) {
        const GComputed& ca = m.computed[k];
        const int csp = m.images[ca.image].space;   // its kernel runs over its image's space
        if (cx.mspace && (csp < 0 || csp >= (int)m.spaces.size() || csp != ca.space)) {
            fprintf(stderr, "[opt_amd] codegen: computed array '%s' carries no index space\n", m.images[ca.image].name.c_str());
            abort();
        }
        o << "extern \"C\" __global__ __launch_bounds__(256) void gen_precompute_" << k << "(GenArgs a) {\n"
          << cx.top_coords() << cx.open_space(csp);
        Body b(cx, o, cx.nd_of(csp));
        const int nch = (int)ca.expr.size();
        for (int ch = 0; ch < nch; ++ch)
            b.line("((T*)a.img[" + std::to_string(ca.image) + "])[lin * " + std::to_string(nch) + " + " + std::to_string(ch) +
                   "] = " + b.v(ca.expr[ch]) + ";");
        for (const GGrad& g : ca.grads)
            if (g.gimg >= 0) b.line("((T*)a.img[" + std::to_string(g.gimg) + "])[lin] = " + b.v(g.expr) + ";");
        o << cx.close_space() << "}\n";
    }
    cx.gs.n_precompute = (int)m.computed.size();
}

// The distinct transcendentals of centred reads in the centred residuals (slot = false) or of
// slot reads in the graph residuals, each with its node at offset 0; like >= 0: only of
// arrays with image `like`'s dims.
using Wanted = std::vector<std::pair<std::tuple<int, int, int>, int>>;
static Wanted wanted_transcendentals(Ctx& cx, bool slot, int like) {
    Pool& P = cx.P;
    Wanted want;
    for (auto& r : cx.m.residuals) {
        if ((r.graph >= 0) != slot) continue;
        P.visit(r.expr, [&](int, const Node& n) {
            if (!cacheable(P, n, slot)) return;
            const Node c = P.at(n.a);
            if (like >= 0 && cx.m.images[c.i].dims != cx.m.images[like].dims) return;
            auto key = std::make_tuple((int)n.op, c.i, c.ch);
            for (auto& w : want)
                if (w.first == key) return;
            const int z0[3] = {0, 0, 0};
            want.push_back({key, P.un(n.op, P.read(c.i, c.ch, z0))});
        });
    }
    return want;
}

// ------------------------------------------------ transcendental caches (see CacheMap)
// Worth it when residuals have instances at several shifts (each would re-evaluate
// its neighbours' transcendentals): cache every sin / cos / exp / log / sqrt / tan /
// atan / ... (transcendental()) of a centred read the residuals use, one internal image
// each, filled by one extra precompute kernel after the ComputedArrays.
void emit_transcendental_cache(Ctx& cx, std::ostringstream& o) {
    GModel& m = cx.m;
    Pool& P = cx.P;
    GenSource& gs = cx.gs;
    CacheMap cache;   // (the kernel that fills it evaluates: cx.cache is set at the end)
    bool multi = false;
    for (auto& r : m.residuals) {
        if (r.graph >= 0) continue;
        std::set<std::string> offs;
        for (int u : r.unknowns) {
            const Node n = P.at(u);
            offs.insert(std::to_string(n.off[0]) + "," + std::to_string(n.off[1]) + "," + std::to_string(n.off[2]));
        }
        multi |= offs.size() > 1;
    }
    const Wanted want = multi && !cx.mspace ? wanted_transcendentals(cx, false, -1) : Wanted{};
    if (!want.empty()) {
        o << "extern \"C\" __global__ __launch_bounds__(256) void gen_precompute_" << gs.n_precompute << "(GenArgs a) {\n"
          << open_owned(cx);
        Body b(cx, o, cx.nd);
        const int uimg = cx.unk.empty() ? 0 : cx.unk[0];
        for (auto& w : want) {
            if (m.images.size() >= 16) break;   // GenArgs::img capacity
            GImage ci;
            ci.name = "cache_" + std::to_string(std::get<0>(w.first)) + "_" + std::to_string(std::get<1>(w.first)) +
                      "_" + std::to_string(std::get<2>(w.first));
            ci.dims = m.images[uimg].dims;
            ci.internal = ci.tvalued = true;
            m.images.push_back(ci);
            const int id = (int)m.images.size() - 1;
            cache[w.first] = id;
            b.line("((T*)a.img[" + std::to_string(id) + "])[lin] = " + b.v(w.second) + ";");
        }
        o << "    }\n}\n";
        if (!cache.empty()) ++gs.n_precompute;
    }
    cx.cache = cache;
}

// predicate cache (see PredCache): up to 8 comparisons of a user array on the unknowns'
// domain with a constant, from the centred residuals and the Exclude expression
void emit_predicate_cache(Ctx& cx, std::ostringstream& o) {
    GModel& m = cx.m;
    Pool& P = cx.P;
    GenSource& gs = cx.gs;
    PredCache pcache;
    const bool on = cx.knobs.pred;
    const int uimg = cx.unk.empty() ? -1 : cx.unk[0];
    auto cmp0 = [](Op op, double l, double r) {
        switch (op) {
            case Op::Lt: return l < r;
            case Op::Le: return l <= r;
            case Op::Gt: return l > r;
            case Op::Ge: return l >= r;
            case Op::Eq: return l == r;
            default: return l != r;
        }
    };
    auto consider = [&](int root) {
        P.visit(root, [&](int, const Node& n) {
            double c;
            bool left;
            int rd;
            if (!pred_form(P, n, &rd, &c, &left)) return;
            const Node r = P.at(rd);
            const GImage& im = m.images[r.i];
            if (im.unknown || im.internal || im.dims != m.images[uimg].dims) return;
            const auto key = std::make_tuple((int)n.op, r.i, r.ch, c, left);
            for (auto& k : pcache.keys)
                if (k == key) return;
            if (pcache.keys.size() >= 8) return;
            pcache.keys.push_back(key);
            pcache.at0.push_back(left ? cmp0(n.op, 0.0, c) : cmp0(n.op, c, 0.0));
        });
    };
    if (on && uimg >= 0 && m.images.size() < 16 && cx.nd == 2 && !cx.mspace) {
        for (auto& r : m.residuals)
            if (r.graph < 0) consider(r.expr);
        if (m.exclude >= 0) consider(m.exclude);
    }
    if (!pcache.keys.empty()) {
        GImage pi;
        pi.name = "pred_bits";
        pi.dims = m.images[uimg].dims;
        pi.internal = true;
        pi.tvalued = false;
        pi.elem = "uint8";
        pi.channels = 1;
        m.images.push_back(pi);
        pcache.img = (int)m.images.size() - 1;
        o << "extern \"C\" __global__ __launch_bounds__(256) void gen_precompute_" << gs.n_precompute << "(GenArgs a) {\n"
          << open_owned(cx);
        Body b(cx, o, cx.nd);
        b.line("unsigned bits = 0;");
        const int z0[3] = {0, 0, 0};
        for (size_t k = 0; k < pcache.keys.size(); ++k) {
            const auto& key = pcache.keys[k];
            const Op op = (Op)std::get<0>(key);
            const int rd0 = P.read(std::get<1>(key), std::get<2>(key), z0), cn = P.cnst(std::get<3>(key));
            const int pn = std::get<4>(key) ? P.bin(op, rd0, cn) : P.bin(op, cn, rd0);
            b.line("bits |= (" + b.cond(pn) + (pcache.at0[k] ? " ? 0u : 1u" : " ? 1u : 0u") + ") << " +
                   std::to_string(k) + ";");
        }
        b.line("((unsigned char*)a.img[" + std::to_string(pcache.img) + "])[lin] = (unsigned char)bits;");
        o << "    }\n}\n";
        ++gs.n_precompute;
    }
    cx.pred = pcache;
}

// graph record cache (see GraphCache): transcendentals of slot reads of arrays on the
// unknowns' domain, one record per vertex, filled by one more precompute kernel
// (several index spaces: one record image and kernel per unknown-carrying space)
void emit_graph_cache(Ctx& cx, std::ostringstream& o) {
    GModel& m = cx.m;
    GenSource& gs = cx.gs;
    std::map<int, GraphCache> gcaches;  // (in use only once every space's kernel is emitted)
    for (int csp : cx.uspaces) {
        GraphCache gcache;
        const bool on = cx.knobs.graph_cache;
        int uimg = -1;
        for (int k : cx.unk)
            if (uimg < 0 && cx.in_space(k, csp)) uimg = k;
        const Wanted want = on && uimg >= 0 && m.images.size() < 16 ? wanted_transcendentals(cx, true, uimg) : Wanted{};
        if (!want.empty()) {
            int width = 1;
            while (width < (int)want.size()) width *= 2;   // aligned records
            GImage ci;
            ci.name = "graph_cache";
            ci.dims = m.images[uimg].dims;
            ci.space = m.images[uimg].space;
            ci.channels = width;
            ci.internal = ci.tvalued = true;
            m.images.push_back(ci);
            gcache.img = (int)m.images.size() - 1;
            gcache.width = width;
            o << "extern \"C\" __global__ __launch_bounds__(256) void gen_precompute_" << gs.n_precompute << "(GenArgs a) {\n"
              << cx.top_coords() << cx.open_space(csp);
            Body b(cx, o, cx.nd_of(csp));
            std::vector<std::string> val(width, "(T)0");
            for (size_t k = 0; k < want.size(); ++k) {
                gcache.ch[want[k].first] = (int)k;
                val[k] = b.v(want[k].second);
            }
            // whole 16-byte vectors per record (width >= 4), scalar stores below that
            const std::string base = "((T*)a.img[" + std::to_string(gcache.img) + "]) + lin * " + std::to_string(width);
            if (width >= 4) {
                for (int g = 0; g < width; g += 4)
                    b.line("*(OptV4*)(" + base + " + " + std::to_string(g) + ") = OptV4{" + val[g] + ", " + val[g + 1] + ", " +
                           val[g + 2] + ", " + val[g + 3] + "};");
            } else {
                for (int k = 0; k < width; ++k) b.line("(" + base + ")[" + std::to_string(k) + "] = " + val[k] + ";");
            }
            o << cx.close_space() << "}\n";
            ++gs.n_precompute;
            gcaches[m.images[uimg].space] = gcache;
        }
    }
    cx.gcache = gcaches;
}

// ---------------------------------------------------------------- gen_jtf
void emit_jtf(Ctx& cx, std::ostringstream& o) {
    GModel& m = cx.m;
    Pool& P = cx.P;
    const std::vector<int>& uslot = cx.uslot;
    auto& inst = cx.inst;
    o << "extern \"C\" __global__ __launch_bounds__(256) void gen_jtf(GenArgs a, T* __restrict__ r, T* __restrict__ diag" << cx.blk_arg() << ") {\n"
      << cx.top_coords();
    for (int sp : cx.uspaces) {
        o << cx.open_space(sp);
        Body b(cx, o, cx.nd_of(sp));
        const int excl = cx.mspace ? m.exclude_of(sp) : m.exclude;
        const std::string act = excl >= 0 ? "(" + b.v(excl) + " == (T)0)" : "true";
        b.line("const bool act = " + act + ";");
        b.line(cx.flag_lin() + " = act ? 1 : 0;");
        for (int k : cx.unk) {
            if (!cx.in_space(k, sp)) continue;
            const GImage& im = m.images[k];
            for (int c = 0; c < im.channels; ++c) {
                std::vector<std::string> F, Dg;
                for (auto& ent : inst[{k, c}]) {
                    const GResidual& r = m.residuals[ent.first.res];
                    const int R = cx.shifted(r.expr, ent.first.s);
                    const int g = cx.shifted(P.diff(r.expr, ent.second), ent.first.s);
                    double gv;
                    if (P.is_const(g, &gv) && gv == 0.0) continue;
                    const std::string gn = b.v(g), rn = b.v(R);
                    F.push_back(gn + " * " + rn);
                    Dg.push_back(gn + " * " + gn);
                }
                const std::string e = "a.uoff[" + std::to_string(uslot[k]) + "] + lin * " + std::to_string(im.channels) +
                                      " + " + std::to_string(c);
                std::string fs = "(T)0", ds = "(T)0";
                for (auto& t : F) fs += " + " + t;
                for (auto& t : Dg) ds += " + " + t;
                b.line("{ const T F = " + fs + "; const T Dg = " + ds + ";");
                b.line("  r[" + e + "] = act ? -F : (T)0; diag[" + e + "] = Dg; }");
            }
        }
        if (cx.blockpre) {
            // every pair of this element's channels: the residual instances containing both
            const int g = cx.group_of(sp);
            std::vector<std::pair<int, int>> rows;   // block row -> (image, channel)
            for (int k : cx.groups[g].images)
                for (int c = 0; c < m.images[k].channels; ++c) rows.push_back({k, c});
            b.line("{ const long long bN = " + cx.blk_n(g) + ", bB = " + cx.blk_base(g) + ";");
            for (int i = 0; i < cx.groups[g].C; ++i)
                for (int j = 0; j <= i; ++j) {
                    std::string s = "(T)0";
                    for (auto& e1 : inst[rows[i]])
                        for (auto& e2 : inst[rows[j]]) {
                            const Instance &I1 = e1.first, &I2 = e2.first;
                            if (I1.res != I2.res || I1.s[0] != I2.s[0] || I1.s[1] != I2.s[1] || I1.s[2] != I2.s[2]) continue;
                            const GResidual& r = m.residuals[I1.res];
                            const int g1 = cx.shifted(P.diff(r.expr, e1.second), I1.s), g2 = cx.shifted(P.diff(r.expr, e2.second), I1.s);
                            double gv;
                            if ((P.is_const(g1, &gv) && gv == 0.0) || (P.is_const(g2, &gv) && gv == 0.0)) continue;
                            s += " + " + b.v(g1) + " * " + b.v(g2);
                        }
                    b.line("  blk[bB + " + std::to_string(tri(i, j)) + "LL * bN + lin] = " + s + ";");
                }
            b.line("}");
        }
        o << cx.close_space();
    }
    o << "}\n";
}

// The nonzero partials of the centred residuals (Entry), their reach and the tile shape of
// gen_apply_tiled; the strips walk the same entries.
void analyse_tiles(Ctx& cx) {
    const GModel& m = cx.m;
    Pool& P = cx.P;
    GenSource& gs = cx.gs;
    auto &cres = cx.cres; auto &ents = cx.ents;
    int &nd_slots = cx.nd_slots, &minx = cx.minx, &maxx = cx.maxx, &miny = cx.miny, &maxy = cx.maxy;
    int &PX = cx.PX, &PY = cx.PY, &TX = cx.TX, &TY = cx.TY, &nf = cx.nf;
    if (gs.has_centered && cx.nd == 2 && !cx.mspace) {
        for (size_t ri = 0; ri < m.residuals.size(); ++ri) {
            const GResidual& r = m.residuals[ri];
            if (r.graph >= 0 || r.unknowns.empty()) continue;
            cres.push_back((int)ri);
            for (int u : r.unknowns) {
                const Node n = P.at(u);
                const int d = P.diff(r.expr, u);
                double gv;
                if (P.is_const(d, &gv) && gv == 0.0) continue;
                Entry e{(int)cres.size() - 1, u, d, P.is_const(d) ? -1 : nd_slots++, n.off[0], n.off[1]};
                ents.push_back(e);
                minx = std::min(minx, n.off[0]); maxx = std::max(maxx, n.off[0]);
                miny = std::min(miny, n.off[1]); maxy = std::max(maxy, n.off[1]);
            }
        }
        // phase 1 covers the tile + halo in exactly one pass of the 256 threads: pick the
        // region shape (32 x 8 or 16 x 16) that leaves the most output pixels
        const int sx = maxx - minx, sy = maxy - miny;
        if ((16 - sx) * (16 - sy) > (32 - sx) * (8 - sy)) PX = PY = 16;
        TX = PX - sx;
        TY = PY - sy;
        nf = (int)cres.size() + nd_slots;
        cx.lds = (size_t)nf * PX * PY * (cx.dbl ? 8 : 4);
        cx.tiled = !cres.empty() && TX > 0 && TY > 0 && cx.lds <= 64 * 1024;
        // the gather evaluates every distinct (residual, shift) instance per pixel; the
        // tiled form evaluates each residual once per centre (+ halo) but pays LDS traffic
        // and barriers. Measured: the gather wins at ~2 instances per
        // residual (image_warping, poisson, optical_flow), the tiles at ~4.7
        // (shape_from_shading, radius-2 supports through ComputedArray gradient images).
        std::set<std::string> inst_keys;
        for (const Entry& e : ents)
            inst_keys.insert(std::to_string(e.r) + ":" + std::to_string(e.ox) + "," + std::to_string(e.oy));
        gs.instances_per_residual = cres.empty() ? 0.0 : (double)inst_keys.size() / cres.size();
        gs.prefer_tiled = cx.tiled && gs.instances_per_residual > 3.0;
    }
}

// -------------------------------------------------------------- gen_apply
// The gather form of the centred J^T J p at pixel `lin` (coordinates in scope). fused:
// inside gen_apply_graph, the sum of output (k, c) goes to cacc<slot>_<c> (declared by
// the caller) instead of Ap
void centred_apply(Ctx& cx, Body& b, bool fused, int sp) {
    const GModel& m = cx.m;
    Pool& P = cx.P;
    const std::vector<int>& uslot = cx.uslot;
    if (!fused) b.line("const bool act = (" + cx.flag_lin() + " & 1) != 0;");
    std::map<std::string, std::string> jp;   // (residual, shift) -> J p of that instance
    for (int k : cx.unk) {
        if (!cx.in_space(k, sp)) continue;
        const GImage& im = m.images[k];
        for (int c = 0; c < im.channels; ++c) {
            std::vector<std::string> terms;
            for (auto& ent : cx.inst[{k, c}]) {
                const GResidual& r = m.residuals[ent.first.res];
                const int* s = ent.first.s;
                const int g = cx.shifted(P.diff(r.expr, ent.second), s);
                double gv;
                if (P.is_const(g, &gv) && gv == 0.0) continue;
                const std::string key = std::to_string(ent.first.res) + ":" + std::to_string(s[0]) + "," +
                                        std::to_string(s[1]) + "," + std::to_string(s[2]);
                if (!jp.count(key)) {
                    std::string sum = "(T)0";
                    for (int u : r.unknowns) {
                        const int gu = cx.shifted(P.diff(r.expr, u), s);
                        if (P.is_const(gu, &gv) && gv == 0.0) continue;
                        sum += " + " + b.v(gu) + " * " + b.vec(cx.shifted(u, s), "p");
                    }
                    const std::string nm = "jp" + std::to_string(jp.size());
                    b.line("const T " + nm + " = " + sum + ";");
                    jp[key] = nm;
                }
                terms.push_back(b.v(g) + " * " + jp[key]);
            }
            std::string acc = "(T)0";
            for (auto& t : terms) acc += " + " + t;
            if (fused) {
                b.line("cacc" + std::to_string(uslot[k]) + "_" + std::to_string(c) + " = " + acc + ";");
                continue;
            }
            const std::string e = "a.uoff[" + std::to_string(uslot[k]) + "] + lin * " + std::to_string(im.channels) +
                                  " + " + std::to_string(c);
            b.line("{ const long long e = " + e + "; const T acc = " + acc + ";");
            b.line("  if (finish) { const T pe = p[e]; const T o = act ? acc + (dadd ? dadd[e] * pe : (T)0) : (T)0; Ap[e] = o; dot += pe * o; }");
            b.line("  else Ap[e] = acc; }");
        }
    }
}
void emit_apply(Ctx& cx, std::ostringstream& o) {
    o << "extern \"C\" __global__ __launch_bounds__(256) void gen_apply(GenArgs a, const T* __restrict__ p, T* __restrict__ Ap,\n"
         "        const T* __restrict__ dadd, const int* stop, ReduceSlot rs, int finish) {\n"
         "    if (stop && *stop) return;\n"
      << cx.top_coords() <<
         "    T dot = 0;\n";
    for (int sp : cx.uspaces) {
        o << cx.open_space(sp);
        Body b(cx, o, cx.nd_of(sp));
        centred_apply(cx, b, false, sp);
        o << cx.close_space();
    }
    o << "    if (finish) { double v[1] = {(double)dot}; block_reduce_publish<1>(v, rs, blockIdx.x); }\n}\n";
}

// ------------------------------------------------------------ gen_apply_tiled
// Two-phase J^T J p over 2-D output tiles whose tile + halo region is 32 x 8 or 16 x 16.
// Phase 1 evaluates every centred residual ONCE per centre q of the tile and the halo
// its outputs gather from: the non-constant partials d(r, u)(q) and Jp_r(q) = sum_u
// d(r, u)(q) p(q + off(u)), kept in LDS. Phase 2 gathers each output x from
// d(r, u)(x - off(u)) * Jp_r(x - off(u)). The gather form of createjtjcentered
// (o.t:2770-2830, what gen_apply does) re-evaluates each residual instance's partials
// for every pixel that reads it; here each is computed once per centre (plus the halo).
void emit_apply_tiled(Ctx& cx, std::ostringstream& o) {
    const GModel& m = cx.m;
    Pool& P = cx.P;
    GenSource& gs = cx.gs;
    const std::vector<int>& uslot = cx.uslot;
    const auto &cres = cx.cres; const auto &ents = cx.ents;
    const int PX = cx.PX, PY = cx.PY, TX = cx.TX, TY = cx.TY, nf = cx.nf, maxx = cx.maxx, maxy = cx.maxy;
    if (!cx.tiled) return;
    gs.has_tiled = true;
    gs.tiles_x = TX;
    gs.tiles_y = TY;
    gs.tiled_lds = cx.lds;
    const int PXY = PX * PY;
    o << "extern \"C\" __global__ __launch_bounds__(256) void gen_apply_tiled(GenArgs a, const T* __restrict__ p, T* __restrict__ Ap,\n"
         "        const T* __restrict__ dadd, const int* stop, ReduceSlot rs, int finish) {\n"
         "    if (stop && *stop) return;\n"
         "    OPT_COORDS\n"
         "    __shared__ T lds[" << nf * PXY << "];\n"
         "    T dot = 0;\n"
         "    const int ntx = (W + " << TX - 1 << ") / " << TX << ", nty = (H + " << TY - 1 << ") / " << TY << ";\n"
         "    for (int t = blockIdx.x; t < ntx * nty; t += gridDim.x) {\n"
         "        const int X0 = (t % ntx) * " << TX << ", Y0 = (t / ntx) * " << TY << ";\n"
         "        for (int idx = threadIdx.x; idx < " << PXY << "; idx += 256) {   // one pass\n"
         "        const int x = X0 - " << maxx << " + idx % " << PX << ", y = Y0 - " << maxy << " + idx / " << PX << ";\n"
         "        const int z = 0; (void)z;\n"
         "        const int li = (y - a.ymem0) * W + x; (void)li;\n"
         "        if (x >= 0 && x < W && y >= 0 && y < H) {\n";
    {
        Body b(cx, o, cx.nd);
        for (size_t ci = 0; ci < cres.size(); ++ci) {
            std::string sum = "(T)0";
            for (size_t ei = 0; ei < ents.size(); ++ei) {
                if (ents[ei].r != (int)ci) continue;
                const std::string dn = b.v(ents[ei].dnode);
                if (ents[ei].slot >= 0)
                    b.line("lds[" + std::to_string((cres.size() + ents[ei].slot) * PXY) + " + idx] = " + dn + ";");
                sum += " + " + dn + " * " + b.vec(ents[ei].u, "p");
            }
            b.line("lds[" + std::to_string(ci * PXY) + " + idx] = " + sum + ";");
        }
    }
    o << "        } else {   // no residual is centred outside the domain (and 0 * stale LDS could be NaN)\n";
    for (int fi = 0; fi < nf; ++fi)
        o << "            lds[" << fi * PXY << " + idx] = (T)0;\n";
    o << "        }\n"
         "        }\n"
         "        __syncthreads();\n"
         "        {\n"
         "        const int lx = threadIdx.x % " << TX << ", ly = threadIdx.x / " << TX << ";\n"
         "        const int x = X0 + lx, y = Y0 + ly;\n"
         "        if (threadIdx.x < " << TX * TY << " && x < W && y < H) {\n"
         "        const long long lin = (long long)(y - a.ymem0) * W + x;\n"
         "        const bool act = (a.flags[lin] & 1) != 0;\n";
    for (int k : cx.unk) {
        const GImage& im = m.images[k];
        for (int c = 0; c < im.channels; ++c) {
            std::string acc = "(T)0";
            for (const Entry& e : ents) {
                const Node n = P.at(e.u);
                if (n.i != k || n.ch != c) continue;
                // centre q = x - off(u), local index in the tile + halo region
                const std::string qi = "(lx + " + std::to_string(maxx - e.ox) + ") + (ly + " +
                                       std::to_string(maxy - e.oy) + ") * " + std::to_string(PX);
                std::string dv;
                if (e.slot >= 0) {
                    dv = "lds[" + std::to_string((cres.size() + e.slot) * PXY) + " + " + qi + "]";
                } else {
                    double cv;
                    P.is_const(e.dnode, &cv);
                    dv = lit(cv);
                }
                acc += " + " + dv + " * lds[" + std::to_string(e.r * PXY) + " + " + qi + "]";
            }
            const std::string el = "a.uoff[" + std::to_string(uslot[k]) + "] + lin * " + std::to_string(im.channels) +
                                   " + " + std::to_string(c);
            o << "        { const long long e = " << el << "; const T acc = " << acc << ";\n"
                 "          if (finish) { const T pe = p[e]; const T o = act ? acc + (dadd ? dadd[e] * pe : (T)0) : (T)0; Ap[e] = o; dot += pe * o; }\n"
                 "          else Ap[e] = acc; }\n";
        }
    }
    o << "        }\n"
         "        }\n"
         "        __syncthreads();\n"
         "    }\n"
         "    if (finish) { double v[1] = {(double)dot}; block_reduce_publish<1>(v, rs, blockIdx.x); }\n}\n";
}

// ------------------------------------------------------------ gen_dump_j_<i>
// saveJToCRS / saveJToCRS_Graph (solverGPUGaussNewton.t:1004-1022, 1287-1305) with
// generateDumpJ (:385-442): the residuals grouped into energy specs by domain in order
// of first appearance (toenergyspecs); element e of spec i owns rows row_base + e R_i +
// r and nonzeros nnz_base + e NNZ_i + ...; each row lists every unknown access of its
// template (zero partials included), column = image offset + channels * tooffset +
// channel wrapped into [0, nUnknowns) (wrap, :365-381), sorted by column (sortCol).
// Every element is written, excluded ones included, as the reference does.
void emit_dump_j(Ctx& cx, std::ostringstream& o) {
    const GModel& m = cx.m;
    Pool& P = cx.P;
    GenSource& gs = cx.gs;
    const std::vector<int>& uslot = cx.uslot;
    const int nd = cx.nd;
    std::vector<int> order;   // spec domains in order of first appearance
    for (auto& r : m.residuals)
        if (std::find(order.begin(), order.end(), r.graph) == order.end()) order.push_back(r.graph);
    if (cx.mspace) order.clear();  // no Jacobian dump over several index spaces (the plan refuses it)
    if (cx.has_loss()) order.clear();  // nor with a RobustEnergy statement (J~ = W J is the plan's own matter)
    for (size_t si = 0; si < order.size(); ++si) {
        const int g = order[si];
        std::vector<const GResidual*> rs;
        int npe = 0;
        for (auto& r : m.residuals)
            if (r.graph == g) { rs.push_back(&r); npe += (int)r.unknowns.size(); }
        gs.dump.push_back({g, (int)rs.size(), npe});
        o << "extern \"C\" __global__ __launch_bounds__(256) void gen_dump_j_" << si
          << "(GenArgs a, int* __restrict__ rowPtr, int* __restrict__ colInd, T* __restrict__ val,\n"
             "        long long row_base, long long nnz_base, long long nunk) {\n"
             "    OPT_COORDS\n";
        if (g < 0) {
            o << "    for (long long lin = a.own_lo + (long long)blockIdx.x * 256 + threadIdx.x; lin < a.own_hi; lin += (long long)gridDim.x * 256) {\n"
              << cx.coords_of(nd) << "        const long long el = lin;\n";
        } else {
            o << "    for (long long el = (long long)blockIdx.x * 256 + threadIdx.x; el < a.nedge[" << g
              << "]; el += (long long)gridDim.x * 256) {\n";
            for (size_t sl = 0; sl < m.graphs[g].slot_names.size(); ++sl)
                o << "        const int v" << sl << " = a.slot[" << gs.slot_base[g] + sl << "][el];\n";
        }
        Body b(cx, o, nd);
        int nz = 0;
        for (size_t ri = 0; ri < rs.size(); ++ri) {
            const GResidual& r = *rs[ri];
            const int K = (int)r.unknowns.size();
            b.line("rowPtr[row_base + el * " + std::to_string(rs.size()) + " + " + std::to_string(ri) +
                   "] = (int)(nnz_base + el * " + std::to_string(npe) + " + " + std::to_string(nz) + ");");
            if (K == 0) continue;
            const std::string cc = "cc" + std::to_string(ri), vv = "vv" + std::to_string(ri);
            b.line("long long " + cc + "[" + std::to_string(K) + "]; T " + vv + "[" + std::to_string(K) + "];");
            int q = 0;
            for (int u : r.unknowns) {
                const Node n = P.at(u);
                const int ch = m.images[n.i].channels;
                std::string idx;
                if (n.slot >= 0) {
                    idx = "(long long)v" + std::to_string(n.slot);
                } else {   // tooffset of the (possibly outside) access
                    idx = "(el + " + std::to_string(n.off[0]) + "LL";
                    if (nd > 1) idx += " + " + std::to_string(n.off[1]) + "LL * W";
                    if (nd > 2) idx += " + " + std::to_string(n.off[2]) + "LL * W * H";
                    idx += ")";
                }
                const int d = P.diff(r.expr, u);
                const std::string dv = b.v(d);
                b.line(cc + "[" + std::to_string(q) + "] = a.uoff[" + std::to_string(uslot[n.i]) + "] + " +
                       std::to_string(ch) + " * " + idx + " + " + std::to_string(n.ch) + "; " + vv + "[" +
                       std::to_string(q) + "] = " + dv + ";");
                ++q;
            }
            const std::string Ks = std::to_string(K);
            b.line("for (int i = 0; i < " + Ks + "; ++i) { const long long c = " + cc + "[i]; " + cc +
                   "[i] = c < 0 ? c + nunk : (c >= nunk ? c - nunk : c); }");
            b.line("for (int i = 1; i < " + Ks + "; ++i) for (int j = i; j > 0 && " + cc + "[j] < " + cc +
                   "[j - 1]; --j) { const long long tc = " + cc + "[j]; " + cc + "[j] = " + cc + "[j - 1]; " + cc +
                   "[j - 1] = tc; const T tv = " + vv + "[j]; " + vv + "[j] = " + vv + "[j - 1]; " + vv + "[j - 1] = tv; }");
            b.line("for (int i = 0; i < " + Ks + "; ++i) { colInd[nnz_base + el * " + std::to_string(npe) + " + " +
                   std::to_string(nz) + " + i] = (int)" + cc + "[i]; val[nnz_base + el * " + std::to_string(npe) +
                   " + " + std::to_string(nz) + " + i] = " + vv + "[i]; }");
            nz += K;
        }
        o << "    }\n}\n";
    }
}

// ------------------------------------------------ RobustEnergy: weights and rho
std::function<std::string(int)> Ctx::weight_at_q(int sbk) const {
    if (!has_loss()) return nullptr;
    return [this, sbk](int group) {
        const auto it = std::find(gs.loss_inc.begin(), gs.loss_inc.end(), std::make_pair(group, sbk));
        if (it == gs.loss_inc.end()) {
            fprintf(stderr, "[opt_amd] codegen: loss group %d has no incidence-order weights at slot %d\n", group, sbk);
            abort();
        }
        const std::string base = "(const T*)a.lwq[" + std::to_string(it - gs.loss_inc.begin()) + "]";
        return off32 ? "opt_g32(" + base + ", q, 1, 0)" : "(" + base + ")[q]";
    };
}
std::function<std::string(int)> Ctx::weight_at_e() const {
    if (!has_loss()) return nullptr;
    return [](int group) { return "((const T*)a.lwe[" + std::to_string(group) + "])[e]"; };
}
// Ceres' definitions on s (Robust losses); neither divides by zero at s = 0:
// Huber's a / sqrt(s) is computed there and not selected
void loss_rho(const Ctx& cx, Body& b, int g, const std::string& s, bool rho) {
    const GLossGroup& L = cx.m.loss[g];
    const std::string G = std::to_string(g), a = "la" + G, a2 = "la2_" + G;
    b.line("const T " + a + " = " + (L.scale_param >= 0 ? "(T)a.prm[" + std::to_string(L.scale_param) + "]" : lit(L.scale)) +
           ", " + a2 + " = " + a + " * " + a + ";");
    if (L.kind == GLossGroup::Huber) {
        b.line("const bool lin" + G + " = " + s + " <= " + a2 + "; const T lr" + G + " = sqrt(" + s + ");");
        b.line("const T rho1" + G + " = lin" + G + " ? (T)1 : " + a + " / lr" + G + ";");
        if (rho) b.line("const T rho" + G + " = lin" + G + " ? " + s + " : (T)2 * " + a + " * lr" + G + " - " + a2 + ";");
    } else {
        b.line("const T lq" + G + " = " + s + " / " + a2 + ";");
        b.line("const T rho1" + G + " = (T)1 / ((T)1 + lq" + G + ");");
        if (rho) b.line("const T rho" + G + " = " + a2 + " * log1p(lq" + G + ");");
    }
}
// s of loss group g at this edge from its raw residuals: declares ls<g>
static void loss_s(Ctx& cx, Body& b, int g) {
    std::string sum = "(T)0";
    for (int f : cx.m.loss[g].raw) {
        const std::string v = b.v(f);
        sum += " + " + v + " * " + v;
    }
    b.line("const T ls" + std::to_string(g) + " = " + sum + ";");
}
// gen_loss_weights: one thread per edge, gen_cost's edge loop. Per loss group: the raw
// residuals, s, w = sqrt(rho'(s)) stored in edge order (lwe) and, once per slot that carries
// unknowns, at the edge's position in that slot's incidence list (lwq through lpos) — the
// gathers then read their weight at q beside gnb[..][q] instead of through geid. With rho1_out
// (OptAMD_EvalLossWeights): rho'(s) of group `only` to the caller's array, the caches untouched.
void emit_loss_weights(Ctx& cx, std::ostringstream& o) {
    const GModel& m = cx.m;
    GenSource& gs = cx.gs;
    if (!cx.has_loss()) return;
    gs.has_loss = true;
    const bool prefetch_nb = cx.knobs.prefetch_nb;
    o << "extern \"C\" __global__ __launch_bounds__(256) void gen_loss_weights(GenArgs a, T* __restrict__ rho1_out, int only) {\n"
      << cx.top_coords();
    for (size_t G = 0; G < m.loss.size(); ++G) {
        const int g = m.loss[G].graph;
        const size_t ns = m.graphs[g].slot_names.size();
        auto sl = [&](size_t s) { return "a.slot[" + std::to_string(gs.slot_base[g] + s) + "]"; };
        o << "    if (only < 0 || only == " << G << ") {\n"
          << "    const long long es = (long long)gridDim.x * 256, ne = a.nedge[" << g << "];\n"
          << "    long long e = opt_xcd_block() * 256 + threadIdx.x;\n";
        if (prefetch_nb)
            for (size_t s = 0; s < ns; ++s) o << "    int n" << s << " = e < ne ? " << sl(s) << "[e] : 0;\n";
        o << "    for (; e < ne; e += es) {\n";
        for (size_t s = 0; s < ns; ++s)
            o << "        const int v" << s << " = " << (prefetch_nb ? "n" + std::to_string(s) : sl(s) + "[e]") << ";\n";
        if (prefetch_nb) {
            o << "        if (e + es < ne) {";
            for (size_t s = 0; s < ns; ++s) o << " n" << s << " = " << sl(s) << "[e + es];";
            o << " }\n";
        }
        Body b(cx, o, cx.nd);
        loss_s(cx, b, (int)G);
        loss_rho(cx, b, (int)G, "ls" + std::to_string(G), false);
        const std::string Gs = std::to_string(G);
        b.line("if (rho1_out) { rho1_out[e] = rho1" + Gs + "; continue; }");
        b.line("const T lw = sqrt(rho1" + Gs + ");");
        b.line("((T*)a.lwe[" + Gs + "])[e] = lw;");
        for (size_t i = 0; i < gs.loss_inc.size(); ++i)
            if (gs.loss_inc[i].first == (int)G)
                b.line("((T*)a.lwq[" + std::to_string(i) + "])[a.lpos[" + std::to_string(gs.loss_inc[i].second) + "][e]] = lw;");
        o << "    }\n    }\n";
    }
    o << "}\n";
}

// ------------------------------------------------------- cost (centres + edges)
void centred_cost_terms(Ctx& cx, Body& b, const std::vector<int>& res) {
    const GModel& m = cx.m;
    std::string sum = "(T)0", ms = "(T)0";
    for (int ri : res) {
        const std::string R = b.v(m.residuals[ri].expr);
        sum += " + " + R + " * " + R;
    }
    b.line("T s = " + sum + ";");
    b.line("if (delta) {");
    for (size_t idx = 0; idx < res.size(); ++idx) {
        const GResidual& r = m.residuals[res[idx]];
        std::string e = b.v(r.expr);
        for (int u : r.unknowns) {
            const int gu = cx.P.diff(r.expr, u);
            double gv;
            if (cx.P.is_const(gu, &gv) && gv == 0.0) continue;
            e += " + " + b.v(gu) + " * " + b.vec(u, "delta");
        }
        b.line("  const T m" + std::to_string(idx) + " = " + e + ";");
        ms += " + m" + std::to_string(idx) + " * m" + std::to_string(idx);
    }
    b.line("  s = " + ms + ";");
    b.line("}");
}
void emit_cost(Ctx& cx, std::ostringstream& o) {
    const GModel& m = cx.m;
    Pool& P = cx.P;
    const GenSource& gs = cx.gs;
    const bool prefetch_nb = cx.knobs.prefetch_nb;
    o << "extern \"C\" __global__ __launch_bounds__(256) void gen_cost(GenArgs a, const T* __restrict__ delta, ReduceSlot rs) {\n"
      << cx.top_coords() <<
         "    T acc = 0;\n";
    for (int sp : cx.uspaces) {
        std::vector<int> here;   // the centred residuals of this space (one space: all of them)
        for (size_t ri = 0; ri < m.residuals.size(); ++ri)
            if (m.residuals[ri].graph < 0 && (!cx.mspace || m.residuals[ri].space == sp)) here.push_back((int)ri);
        if (here.empty()) continue;
        o << cx.open_space(sp);
        Body b(cx, o, cx.nd_of(sp));
        const int excl = cx.mspace ? m.exclude_of(sp) : m.exclude;
        if (excl >= 0) b.line("if (" + b.v(excl) + " != (T)0) continue;");
        centred_cost_terms(cx, b, here);
        b.line("acc += (T)0.5 * s;");
        o << cx.close_space();
    }
    for (size_t g = 0; g < m.graphs.size(); ++g) {
        bool any = false;
        for (auto& r : m.residuals) any |= r.graph == (int)g;
        if (!any) continue;
        // the next edge's vertex ids are loaded one edge ahead (as the gathers' edge loops)
        const size_t ns = m.graphs[g].slot_names.size();
        auto sl = [&](size_t s) { return "a.slot[" + std::to_string(gs.slot_base[g] + s) + "]"; };
        o << "    {\n    const long long es = (long long)gridDim.x * 256, ne = a.nedge[" << g << "];\n"
          << "    long long e = opt_xcd_block() * 256 + threadIdx.x;\n";
        if (prefetch_nb)
            for (size_t s = 0; s < ns; ++s) o << "    int n" << s << " = e < ne ? " << sl(s) << "[e] : 0;\n";
        o << "    for (; e < ne; e += es) {\n";
        for (size_t s = 0; s < ns; ++s)
            o << "        const int v" << s << " = " << (prefetch_nb ? "n" + std::to_string(s) : sl(s) + "[e]") << ";\n";
        if (prefetch_nb) {
            o << "        if (e + es < ne) {";
            for (size_t s = 0; s < ns; ++s) o << " n" << s << " = " << sl(s) << "[e + es];";
            o << " }\n";
        }
        Body b(cx, o, cx.nd);
        std::string sum = "(T)0";
        // RobustEnergy: per loss group of this graph s, rho(s), rho'(s) from the raw residuals and
        // w recomputed inline (the expression gen_loss_weights caches). Its templates W f_k then
        // go through the same q_k as the plain ones; their squares are summed apart (lsum): the
        // cost takes rho(s), the model cost rho(s) - rho'(s) s + sum_k (f~_k + J~_k delta)^2
        std::string lsum = "(T)0", lrho = "(T)0", lconst = "(T)0";
        bool lossy = false;
        for (size_t G = 0; G < m.loss.size(); ++G) {
            if (m.loss[G].graph != (int)g) continue;
            const std::string Gs = std::to_string(G);
            lossy = true;
            loss_s(cx, b, (int)G);
            loss_rho(cx, b, (int)G, "ls" + Gs, true);
            b.line("const T lw" + Gs + " = sqrt(rho1" + Gs + ");");
            lrho += " + rho" + Gs;
            lconst += " + (rho" + Gs + " - rho1" + Gs + " * ls" + Gs + ")";
        }
        if (lossy) b.weight_at([](int G) { return "lw" + std::to_string(G); });
        int idx = 0;
        for (size_t ri = 0; ri < m.residuals.size(); ++ri) {
            const GResidual& r = m.residuals[ri];
            if (r.graph != (int)g) continue;
            std::string e = b.v(r.expr);
            b.line("T q" + std::to_string(idx) + " = " + e + ";");
            (lossy && m.loss_group_of((int)ri) >= 0 ? lsum : sum) += " + q" + std::to_string(idx) + " * q" + std::to_string(idx);
            ++idx;
        }
        b.line("if (delta) {");
        idx = 0;
        for (auto& r : m.residuals) {
            if (r.graph != (int)g) continue;
            std::string e;
            for (int u : r.unknowns) {
                const int gu = P.diff(r.expr, u);
                double gv;
                if (P.is_const(gu, &gv) && gv == 0.0) continue;
                e += " + " + b.v(gu) + " * " + b.vec(u, "delta");
            }
            if (!e.empty()) b.line("  q" + std::to_string(idx) + " = q" + std::to_string(idx) + e + ";");
            ++idx;
        }
        b.line("}");
        b.line("acc += (T)0.5 * (" + sum + ");");
        if (lossy) b.line("acc += (T)0.5 * (delta ? " + lconst + " + " + lsum + " : " + lrho + ");");
        o << "    }\n    }\n";
    }
    o << "    double v[1] = {(double)acc};\n    block_reduce_publish<1>(v, rs, blockIdx.x);\n}\n";
}

GenSource generate(GModel& m, bool dbl, bool off32) {
    GenSource gs;
    Ctx cx(m, dbl, off32, read_knobs(), gs);
    int sb = 0;
    for (size_t g = 0; g < m.graphs.size() && g < 4; ++g) {
        gs.slot_base[g] = sb;
        sb += (int)m.graphs[g].slot_names.size();
    }
    for (auto& r : m.residuals) (r.graph < 0 ? gs.has_centered : gs.has_graph) = true;
    // RobustEnergy: one incidence-order weights array per (group, slot through which one of the
    // group's residuals reads an unknown): the slots whose gathers evaluate the group
    for (size_t G = 0; G < m.loss.size(); ++G)
        for (int ri : m.loss[G].residuals)
            for (int u : m.residuals[ri].unknowns) {
                const std::pair<int, int> key((int)G, gs.slot_base[m.loss[G].graph] + m.pool.at(u).slot);
                if (std::find(gs.loss_inc.begin(), gs.loss_inc.end(), key) == gs.loss_inc.end()) gs.loss_inc.push_back(key);
            }
    std::sort(gs.loss_inc.begin(), gs.loss_inc.end());

    std::ostringstream o;
    emit_prelude(cx, o);
    emit_precompute(cx, o);
    emit_transcendental_cache(cx, o);
    emit_predicate_cache(cx, o);
    emit_graph_cache(cx, o);
    emit_jtf(cx, o);
    analyse_tiles(cx);
    emit_apply(cx, o);
    emit_apply_tiled(cx, o);
    if (cx.tiled) emit_strips(cx, o);
    emit_dump_j(cx, o);
    emit_cost(cx, o);
    emit_loss_weights(cx, o);
    emit_graph_gathers(cx, o);
    emit_block_pcg(cx, o);
    emit_schur(cx, o);
    emit_schur_explicit(cx, o);
    emit_normal(cx, o);
    char note[128];
    snprintf(note, sizeof(note), "// apply: %s (%.2f residual instances per centred residual)\n",
             gs.has_strip ? "gen_apply_strip" : gs.prefer_tiled ? "gen_apply_tiled" : "gen_apply",
             gs.instances_per_residual);
    gs.code = note + o.str();
    return gs;
}

}  // namespace gen
}  // namespace optamd
