// gen/codegen_ctx.h — internal to the generator (codegen*.cpp): the per-call context every
// emitter works over, the Body expression emitter, and the emitters themselves. All state
// of one generate() call lives in its Ctx, so calls on different models may run at once.
#pragma once
#include <functional>
#include <map>
#include <set>
#include <sstream>
#include <tuple>
#include "codegen.h"

namespace optamd {
namespace gen {

// The OPT_AMD_GEN_* environment knobs, read once per generate() call (read_knobs).
struct Knobs {
    // the register-strip kernels' row loads / stores through 32-bit offsets (with off32):
    // OPT_AMD_GEN_STRIP32=0 64-bit element indices, 1 32-bit, 2 32-bit kept opaque (opt_o32),
    // 4 (default) opaque in the kernels without two-channel pair reads
    int strip32 = 4;
    // OPT_AMD_GEN_WIDU: the strip kernels' wave index through readfirstlane (row indices and
    // bounds in SGPRs): 0 never, 1 always, 2 (default) in the kernels without pair windows
    int widu = 2;
    // OPT_AMD_GEN_FACTOR=0: the strip apply masks every partial of a masked residual (else the
    // residual's mask once, on Jp)
    bool factor = true;
    // graph edge loops: vertex ids one edge ahead (OPT_AMD_GEN_NB_PREFETCH=0: at use)
    bool prefetch_nb = true;
    // OPT_AMD_GEN_EDGE_UNROLL=k: unroll the gathers' edge loops k times
    // (generated ARAP 1M vertices, profiles/r03_unroll_ab.json: apply 89 / 82-83 / 81 us at
    // 1 / 2 / 4, GN step 1.63 / 1.63 / 1.56-1.58 ms; 4 by default, 1 = no pragma)
    int edge_unroll = 4;
    bool pred = true;          // OPT_AMD_GEN_PRED=0: no predicate cache (PredCache)
    bool graph_cache = true;   // OPT_AMD_GEN_GRAPH_CACHE=0: no graph record cache (GraphCache)
};

// Per-step caches of single-pixel transcendentals: (op, image, channel) -> internal image
// holding op(image(x).channel) for every pixel, refreshed by the last precompute kernel.
// Once built, the emitter reads f(image(x + o)) from the cache at offset o instead of
// evaluating it (the gather evaluates each residual instance, so an angle's sin/cos would
// otherwise be recomputed at every neighbour that reads it). Same function, same input:
// the cached values are the bits the kernels would compute.
using CacheMap = std::map<std::tuple<int, int, int>, int>;
// Per-step predicate cache (the register strips): comparisons of a centred read of a user
// array with a constant (Mask == 0, Constraints >= 0, ...) packed as bits of one uint8
// image, filled by a precompute kernel once per Step — a strip reads one byte per pixel
// instead of the arrays the masks test. Bit k holds pred_k(v) XOR pred_k(0), so the 0 a
// window reads outside the image decodes to pred_k(0), the value the uncached expression
// gives there. Key: (op, image, channel, constant, read on the left).
struct PredCache {
    int img = -1;
    std::vector<std::tuple<int, int, int, double, bool>> keys;
    std::vector<bool> at0;   // pred_k(0)
};
// Graph energies: the same values for slot reads, packed per vertex into one record image
// (channel k of the record = key k) — a gather pass evaluates every incident edge, so the
// other slot's sin / cos would be re-evaluated once per edge (ARAP's angles: three
// sincos per edge in the reverse pass); the record is one 32-byte line per vertex.
struct GraphCache {
    int img = -1, width = 0;
    std::map<std::tuple<int, int, int>, int> ch;
};

struct Instance {   // a centred residual shifted so that it contains unknown (image, ch) at 0
    int res;
    int s[3];
};
// a nonzero partial d(residual cres[r]) / d(unknown access u) of the tiled / strip forms
struct Entry { int r; int u; int dnode; int slot; int ox, oy; };   // slot -1: constant partial

// What the emitters share about the model, computed once per call. The first group is
// filled by the constructor (it reads the pool without growing it); the tile group by
// analyse_tiles() after gen_jtf, where its P.diff calls have always happened (pool order is
// part of the output: node ids appear in the emitted names).
struct Analysis {
    explicit Analysis(const GModel& m);
    int nd;                       // dimensionality of the (first) unknowns' index space
    std::vector<int> unk, uslot;  // unknown image ids; image id -> position among them (-1)
    // centred instances per output (unknown image, channel) -> (instance, support node)
    std::map<std::pair<int, int>, std::vector<std::pair<Instance, int>>> inst;
    // Kernel loops over the elements of an index space. One space (every energy until
    // bundle_adjustment.t / row_bias.t): the owned pixels of the unknowns' domain, a.dims.
    // Several (mspace): one grid-stride loop per space inside the same kernel, W / H / D and
    // the flag base fb taken from that space's GenArgs entries; such energies run the gather
    // forms only (no strips, tiles, slabs or Jacobian dump).
    bool mspace;
    std::vector<int> uspaces;
    // Block preconditioner (UsePreconditioner("block")): the kernels that build J^T F also
    // accumulate, per element of every unknown-carrying space, the packed lower triangle of
    // that element's diagonal block of J^T J: blk[base_g + j * N_g + e], entry j slowest.
    bool blockpre;
    std::vector<GBlockGroup> groups;
    // Eliminate (GModel::eliminated): the eliminated group among `groups`, -1 without the
    // statement; PCG runs on the Schur complement over the other groups (codegen_schur.cpp)
    int elim_group;

    // the tiled / strip forms (2-D centred, one space; analyse_tiles)
    std::vector<int> cres;        // centred residual ids
    std::vector<Entry> ents;
    int nd_slots = 0;
    int minx = 0, maxx = 0, miny = 0, maxy = 0;
    int PX = 32, PY = 8, TX = 0, TY = 0, nf = 0;
    size_t lds = 0;
    bool tiled = false;
};

struct Ctx : Analysis {
    Ctx(GModel& model, bool dbl_, bool off32_, const Knobs& k, GenSource& out)
        : Analysis(model), m(model), P(model.pool), dbl(dbl_), off32(off32_), knobs(k), gs(out) {}
    GModel& m;
    Pool& P;
    const bool dbl;
    // Slot reads (graph gathers) as uniform base + 32-bit byte offset (generate's off32): the
    // saddr form of global_load, one 32-bit multiply per neighbour instead of a 64-bit address
    // per gathered array
    const bool off32;
    const Knobs knobs;
    GenSource& gs;
    // set by their builders (emit_*_cache) once the kernel that fills them is emitted
    CacheMap cache;
    PredCache pred;
    std::map<int, GraphCache> gcache;   // one per index space whose arrays the slot reads' transcendentals are of

    bool s32() const { return off32 && knobs.strip32 != 0; }
    int shifted(int id, const int* s) const { return P.shift(id, s); }
    int nd_of(int sp) const { return mspace ? (int)m.spaces[sp].size() : nd; }
    const char* coords_of(int ndim) const;   // memory pixel index `lin` -> x, y, z, li
    std::string top_coords() const { return mspace ? "" : "    OPT_COORDS\n"; }
    std::string open_space(int sp) const;    // the element loop of space sp, coordinates in scope
    std::string close_space() const { return mspace ? "    }\n    }\n" : "    }\n"; }
    std::string flag_lin() const { return mspace ? "a.flags[fb + lin]" : "a.flags[lin]"; }
    bool in_space(int image, int sp) const { return !mspace || m.images[image].space == sp; }
    // block groups: the group of a space, its element count, first entry, row of a channel
    int group_of(int sp) const;
    std::string blk_n(int g) const;
    std::string blk_base(int g) const;
    int blk_row(int g, int image, int ch) const;
    std::string blk_arg() const { return blockpre ? ", T* __restrict__ blk" : ""; }
    // Schur kernels: the eliminated space, and where a read of the PCG vector `vname` at
    // unknown image `image` starts (set by the Schur emitters while they emit: the eliminated
    // images of "w" start inside the compact scratch vector; unset: vname + a.uoff[image])
    bool schur() const { return elim_group >= 0; }
    int elim_space() const { return groups[elim_group].space; }
    std::function<std::string(int image, const char* vname)> vec_base;
    // RobustEnergy (GModel::loss): the weight loads of a Body (Body::weight_at). weight_at_q: the
    // gather over GenArgs::slot index sbk reads GenArgs::lwq[i][q], i the place of (group, sbk)
    // in GenSource::loss_inc; weight_at_e: a per-edge kernel reads GenArgs::lwe[group][e]
    bool has_loss() const { return !m.loss.empty(); }
    std::function<std::string(int)> weight_at_q(int sbk) const;
    std::function<std::string(int)> weight_at_e() const;
};
inline int tri(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }

std::string lit(double v);
const char* elem_type(const std::string& e, bool unknown);
bool cacheable(const Pool& P, const Node& n, bool slot);   // transcendental of a centred / slot read
// n compares a centred read (*rd) with a constant (*c); *left: the read is the left operand
bool pred_form(const Pool& P, const Node& n, int* rd, double* c, bool* left);
// bit index of predicate node n (and its Read child), -1 when n is not a cached predicate
int pred_bit(const Ctx& cx, const Node& n, int* rd);

// One kernel body's emitter: every pool node becomes at most one local temporary.
class Body {
public:
    Body(const Ctx& cx, std::ostringstream& o, int ndims) : C_(cx), M_(cx.m), P_(cx.P), o_(o), nd_(ndims) {}

    // Graph gathers: nodes that read only the gathering vertex's own slot (`self`), params
    // and constants are the same for every incident edge; they go to `pre`, emitted before
    // the edge loop (the vertex's own sin/cos, unknowns and knowns once per vertex instead
    // of once per edge).
    void hoist_to(std::ostringstream* pre, int self, int graph) { pre_ = pre; self_ = self; graph_ = graph; }
    std::string v(int id);      // node `id` as a T value (the name of its temporary)
    // node `id` as a C++ condition (nonzero)
    std::string cond(int id) { return is_bool(id) ? bv(id) : "(" + v(id) + " != (T)0)"; }
    std::string bv(int id);     // the bool value of boolean node `id`
    // the search direction / step vector at unknown access `u` (a Read of an unknown)
    std::string vec(int u, const char* vname);
    void line(const std::string& s) { o_ << "        " << s << "\n"; }
    // the strip kernels read cached predicates (Ctx::pred) from the bit image's row windows
    void use_pred(bool on) { use_pred_ = on; }
    // ... and take sin / cos of a window value: no transcendental cache images (Ctx::cache)
    void use_cache(bool on) { use_cache_ = on; }
    // register-strip emission (RowWindows): centred reads come from the caller's row
    // windows instead of memory
    void centred_reads(std::function<std::string(const Node&, const char*)> f) { centred_ = std::move(f); }
    // RobustEnergy: where this body reads loss group g's weight (Op::Weight) — the incidence-order
    // copy at q in a gather, the edge-order copy at e in a per-edge kernel (Ctx::weight_at_q /
    // weight_at_e), or a value the kernel has computed itself (gen_cost)
    void weight_at(std::function<std::string(int)> f) { weight_ = std::move(f); }

private:
    bool invariant(int id);
    std::ostream& out(int id) { return invariant(id) ? static_cast<std::ostream&>(*pre_) : o_; }
    bool is_bool(int id);
    std::string coord(int k, int off) const;
    std::string inb(const int* off) const;
    std::string inbox(const int* lo, const int* hi) const { return "(" + inb(lo) + ") && (" + inb(hi) + ")"; }
    std::string rel(const int* off) const;
    std::string img_ptr(int i) const;
    std::string read(const Node& n, const char* vname);

    const Ctx& C_;
    GModel& M_;
    Pool& P_;
    std::ostringstream& o_;
    int nd_;
    std::map<int, std::string> done_, bdone_;
    std::map<int, bool> isb_;
    bool use_pred_ = false, use_cache_ = true;
    std::set<int> sincos_, rec_;
    std::map<std::string, std::string> vdone_;
    std::ostringstream* pre_ = nullptr;
    int self_ = -1, graph_ = -1;
    std::map<int, bool> inv_;
    std::function<std::string(const Node&, const char*)> centred_;
    std::function<std::string(int)> weight_;
};

// The emitters, in emission order (generate() calls them so; each appends its kernels to o).
void emit_prelude(const Ctx& cx, std::ostringstream& o);             // typedefs, GenArgs, opt_* device helpers
void emit_precompute(Ctx& cx, std::ostringstream& o);                // gen_precompute_<k>: ComputedArrays
void emit_transcendental_cache(Ctx& cx, std::ostringstream& o);      // Ctx::cache and its precompute kernel
void emit_predicate_cache(Ctx& cx, std::ostringstream& o);           // Ctx::pred ...
void emit_graph_cache(Ctx& cx, std::ostringstream& o);               // Ctx::gcache ...
void emit_jtf(Ctx& cx, std::ostringstream& o);                       // gen_jtf
void analyse_tiles(Ctx& cx);                                         // Analysis' tile group, gs.prefer_tiled
void centred_apply(Ctx& cx, Body& b, bool fused, int sp);            // gen_apply's body (and the fused graph apply's)
void emit_apply(Ctx& cx, std::ostringstream& o);                     // gen_apply
void emit_apply_tiled(Ctx& cx, std::ostringstream& o);               // gen_apply_tiled
void emit_strips(Ctx& cx, std::ostringstream& o);                    // gen_apply_strip, gen_jtf_strip, gen_cost_strip
void emit_dump_j(Ctx& cx, std::ostringstream& o);                    // gen_dump_j_<i>
// gen_cost's per-centre terms over residuals `res`: T s = sum r^2, or with delta sum (r + J delta)^2
void centred_cost_terms(Ctx& cx, Body& b, const std::vector<int>& res);
void emit_cost(Ctx& cx, std::ostringstream& o);                      // gen_cost
void emit_loss_weights(Ctx& cx, std::ostringstream& o);              // gen_loss_weights (RobustEnergy)
// loss group g at an edge whose raw residuals' squares sum to `s` (a T temporary): declares
// rho1<g> = rho'(s) and, with `rho`, rho<g> = rho(s)
void loss_rho(const Ctx& cx, Body& b, int g, const std::string& s, bool rho);
void emit_graph_gathers(Ctx& cx, std::ostringstream& o);             // gen_jtf_graph, gen_apply_graph
void emit_block_pcg(const Ctx& cx, std::ostringstream& o);           // gen_blk_*
// One vertex's gather over its incidence lists (codegen_graph.cpp): J^T F's terms, or with
// `apply` J^T J p's. schur 1: p read at the retained images only (E^T p_r at a vertex of the
// eliminated space); 2: eliminated images read from "w" instead of "p"
void graph_gather(Ctx& cx, std::ostringstream& o, bool apply, int sp, int schur = 0);
void emit_schur(Ctx& cx, std::ostringstream& o);                     // gen_schur_rhs, gen_schur_elim, gen_schur_apply
void emit_schur_explicit(Ctx& cx, std::ostringstream& o);            // gen_schur_eblk, gen_schur_assemble, gen_schur_spmv
// shared by the two explicitly formed matrices (codegen_schur_explicit.cpp): the pair-list
// assembly kernels `name` / `name`_long, and opt_rbase / opt_rstride, the place of a block
// group's rows in the unknown vector
void emit_pair_assemble(std::ostringstream& o, const std::string& name, int CR, int CE, const std::string& Gr, bool minus,
                        bool packed = false);
void emit_group_rows(const Ctx& cx, std::ostringstream& o, const GBlockGroup& GR);
void emit_dense(Ctx& cx, std::ostringstream& o, const std::string& Gr, int C);   // gen_dense_fill, gen_dense_store (LinearSolver("cholesky"))
void emit_normal(Ctx& cx, std::ostringstream& o);                    // gen_normal_eblk, gen_normal_assemble, gen_normal_spmv

}  // namespace gen
}  // namespace optamd
