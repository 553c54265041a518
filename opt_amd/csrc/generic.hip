// generic.hip — the general energy path: any energy file the front end (gen/) lowers,
// solved by the same GN / LM driver (stencil_plan.h) with kernels generated for that
// energy and compiled at plan time with hiprtc for gfx950.
//
// This is the role of the reference's whole compile pipeline (problemSpecFromFile →
// toenergyspecs → createfunctionset → solverGPUGaussNewton's kernels, API/src/o.t:
// 1295-1348, 2669-3235). The hand-written families (image_warping.hip, ...) remain the
// fast paths for the energies they recognise; this path covers every other energy in
// the DSL subset gen/lua.cpp accepts (centred stencils over 1-3-D index spaces, graph
// residuals, Exclude, Select / InBounds, scalar parameters, up to 4 unknown images, which
// may lie over several index spaces: cameras / points / observations).
// OPT_AMD_GENERIC=1 routes recognised families here too (to validate it against the
// hand-written kernels and the reference's known answers).
#include <hip/hiprtc.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include "explicit_matrix.h"
#include "gen/codegen.h"
#include "graph_util.h"
#include "stencil_plan.h"

namespace optamd {

namespace {

#define OPT_RTC_CHECK(call)                                                                          \
    do {                                                                                             \
        hiprtcResult r_ = (call);                                                                    \
        if (r_ != HIPRTC_SUCCESS) {                                                                  \
            fprintf(stderr, "[opt_amd] hiprtc error %d (%s) in %s\n", (int)r_, hiprtcGetErrorString(r_), #call); \
            exit(1);                                                                                 \
        }                                                                                            \
    } while (0)

// Compile `code` to a gfx950 code object. false + log on a compile error.
bool rtc_compile(const std::string& code, std::string* obj, std::string* log) {
    hiprtcProgram prog;
    OPT_RTC_CHECK(hiprtcCreateProgram(&prog, code.c_str(), "opt_amd_generic.hip", 0, nullptr, nullptr));
    const char* opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17"};
    const hiprtcResult rc = hiprtcCompileProgram(prog, 3, opts);
    size_t n = 0;
    hiprtcGetProgramLogSize(prog, &n);
    if (n > 1) {
        log->resize(n);
        hiprtcGetProgramLog(prog, &(*log)[0]);
    }
    if (rc != HIPRTC_SUCCESS) {
        hiprtcDestroyProgram(&prog);
        return false;
    }
    OPT_RTC_CHECK(hiprtcGetCodeSize(prog, &n));
    obj->resize(n);
    OPT_RTC_CHECK(hiprtcGetCode(prog, &(*obj)[0]));
    hiprtcDestroyProgram(&prog);
    return true;
}

// Process-wide cache: one code object per distinct generated source.
std::mutex g_mu;
std::map<std::string, std::string>& code_cache() {
    static std::map<std::string, std::string> m;
    return m;
}

__global__ void incidence_count(const int* keys, int E, int* counts) {
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < E; e += gridDim.x * blockDim.x)
        atomicAdd(&counts[keys[e]], 1);
}
// out[q] = slot[geid[q]]: one slot's vertex of each edge of an incidence list, in its order
__global__ void incidence_gather(const int* slot, const int* geid, int E, int* out) {
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < E; q += gridDim.x * blockDim.x) out[q] = slot[geid[q]];
}
// pos[geid[q]] = q: where each edge sits in an incidence list (geid is a permutation of [0, E))
__global__ void incidence_positions(const int* geid, int E, int* pos) {
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < E; q += gridDim.x * blockDim.x) pos[geid[q]] = q;
}
__global__ void iota_kernel(int* v, int n) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) v[i] = i;
}

size_t elem_size(const gen::GImage& im, bool dbl) {
    if (im.tvalued) return dbl ? 8 : 4;
    if (im.elem == "uint8") return 1;
    return 4;
}

// gen::generate's off32: every array the graph gathers read is below 2 GiB — the unknown
// vectors, the images (all allocated at the unknowns' domain size), the graph record cache
// (at most 16 fields per vertex in the 32-bit form, codegen.cpp) and the per-edge
// incidence copies. The same answer at the admission compile and in the plan.
bool gather_offsets_fit_32(const gen::GModel& m, const ProblemSpec& s, bool dbl) {
    if (env_int("OPT_AMD_GEN_OFF32", 1) == 0) return false;   // tests: force the 64-bit form
    const long long lim = 1LL << 31, t = dbl ? 8 : 4;
    auto pixels = [&](const std::vector<int>& dims) {
        long long n = 1;
        for (int d : dims) n *= (long long)s.dim_values.at(m.dims[d].index);
        return n;
    };
    long long npix = 0, total = 0;   // the largest unknown-carrying space, the whole unknown vector
    for (int k : m.unknown_images()) {
        npix = std::max(npix, pixels(m.images[k].dims));
        total += pixels(m.images[k].dims) * m.images[k].channels;
    }
    bool ok = total * t < lim && npix * 16 * t < lim;
    for (auto& im : m.images) ok &= pixels(im.dims) * im.channels * (long long)elem_size(im, dbl) < lim;
    for (auto& g : m.graphs) {
        long long e = 1;
        for (int d : g.dims) e *= (long long)s.dim_values.at(m.dims[d].index);
        ok &= e * 4 < lim;
    }
    return ok;
}

}  // namespace

// Front-end admission check for Opt_ProblemDefine: lower the energy and check it fits the
// generated kernels' limits. Fills the spec fields the driver reads.
bool generic_accepts(const std::string& text, ProblemSpec* spec, std::string* err) {
    gen::GModel m;
    if (!gen::build_model(text, &m, err)) return false;
    if (!m.unsupported.empty()) {
        *err = "the general front end does not lower '" + m.unsupported + "'";
        return false;
    }
    const std::vector<int> unk = m.unknown_images();
    if (unk.empty()) { *err = "no Unknown declared"; return false; }
    if (m.unknown_spaces().size() > 4) { *err = "more than 4 index spaces hold unknowns"; return false; }
    if (m.spaces.size() > 8) { *err = "more than 8 index spaces"; return false; }
    if (unk.size() > 4) { *err = "more than 4 unknown images"; return false; }
    if (m.images.size() > 16) { *err = "more than 16 images"; return false; }
    if (m.params.size() > 32) { *err = "more than 32 parameters"; return false; }
    if (m.graphs.size() > 4) { *err = "more than 4 graphs"; return false; }
    size_t slots = 0;
    for (auto& g : m.graphs) slots += g.slot_names.size();
    if (slots > 16) { *err = "more than 16 graph vertex arrays"; return false; }
    for (auto& sp : m.spaces)
        if (sp.size() < 1 || sp.size() > 3) { *err = "index spaces must be 1-, 2- or 3-dimensional"; return false; }
    if (m.residuals.empty()) { *err = "no Energy terms"; return false; }
    {   // RobustEnergy: one incidence-order weights array per (group, slot that carries its unknowns)
        size_t arrays = 0;
        for (auto& L : m.loss) {
            std::vector<int> sl;
            for (int ri : L.residuals)
                for (int u : m.residuals[ri].unknowns)
                    if (std::find(sl.begin(), sl.end(), m.pool.at(u).slot) == sl.end()) sl.push_back(m.pool.at(u).slot);
            arrays += sl.size();
        }
        if (arrays > 16) { *err = "RobustEnergy: more than 16 (loss group, graph slot) weight arrays"; return false; }
    }
    if (m.block_preconditioner)
        for (auto& g : m.block_groups())
            if (g.C > 8) {
                std::string sn = "{";
                for (size_t k = 0; k < m.spaces[g.space].size(); ++k) sn += (k ? "," : "") + m.dims[m.spaces[g.space][k]].name;
                *err = "UsePreconditioner(\"block\"): index space " + sn + "} holds " + std::to_string(g.C) +
                       " unknown channels (a block has at most 8)";
                return false;
            }
    spec->text = text;
    spec->use_preconditioner = m.use_preconditioner;
    spec->block_preconditioner = m.block_preconditioner;
    spec->eliminate.clear();
    for (int k : m.eliminated) spec->eliminate.push_back(m.images[k].name);
    spec->family = "generic";
    return true;
}

// Structural signature of a lowered energy: every declaration (kind, element type,
// channels, index space, problemparams index — names dropped) and every residual,
// ComputedArray and exclusion template as the hash-consed pool prints it. Two energy
// files with equal signatures define the same problem and the same derivatives
// (the reference derives all kernels from exactly these, o.t:1295-1348, 2669-2715).
bool generic_signature(const std::string& text, std::string* sig, bool* use_pre, std::string* err) {
    gen::GModel m;
    if (!gen::build_model(text, &m, err)) return false;
    if (!m.unsupported.empty()) { *err = "unsupported: " + m.unsupported; return false; }
    std::string s;
    auto ids = [](const std::vector<int>& v) {
        std::string o;
        for (int x : v) o += std::to_string(x) + ",";
        return o;
    };
    for (auto& d : m.dims) s += "D" + std::to_string(d.index) + ";";
    for (auto& im : m.images)
        s += "I" + std::to_string(im.index) + ":" + std::to_string(im.channels) + (im.unknown ? "u" : "a") +
             (im.internal ? "i" : "") + (im.tvalued ? "t" : "") + im.elem + "{" + ids(im.dims) + "};";
    for (auto& p : m.params) s += "P" + std::to_string(p.index) + ":" + p.type + ";";
    // (slot spaces, residual and Exclude spaces: only for energies over several index spaces,
    // so that a single-space energy's signature is what it always was)
    for (auto& g : m.graphs)
        s += "G{" + ids(g.dims) + "}{" + ids(g.slot_index) + "}" + (m.multi() ? "{" + ids(g.slot_space) + "}" : "") + ";";
    for (auto& c : m.computed) {
        s += "C" + std::to_string(c.image) + ":";
        for (int e : c.expr) s += m.pool.str(e) + "|";
        std::vector<std::string> gs;   // a set: its order follows traversal, not meaning
        for (auto& g : c.grads)
            gs.push_back("g" + std::to_string(g.ch) + "," + (g.u >= 0 ? m.pool.str(g.u) : std::string("-")) + "," +
                         (g.gimg >= 0 ? "img," : "const,") + (g.expr >= 0 ? m.pool.str(g.expr) : std::string("-")) + "|");
        std::sort(gs.begin(), gs.end());
        for (auto& g : gs) s += g;
        for (int k = 0; k < 3; ++k) s += std::to_string(c.lo[k]) + ":" + std::to_string(c.hi[k]) + ",";
        s += ";";
    }
    if (!m.multi()) s += "X" + (m.exclude >= 0 ? m.pool.str(m.exclude) : std::string("-")) + ";";
    for (auto& x : m.excludes)
        if (m.multi()) s += "X" + std::to_string(x.first) + ":" + m.pool.str(x.second) + ";";
    for (auto& r : m.residuals)
        s += "R" + std::to_string(r.graph) + (m.multi() && r.graph < 0 ? "s" + std::to_string(r.space) : "") + ":" +
             std::to_string(r.unknowns.size()) + ":" + m.pool.str(r.expr) + ";";
    // (only when requested: every other energy's signature is what it always was)
    if (m.block_preconditioner) s += "B;";
    // NormalMatrix("explicit"): the normal matrix's form ("matrix_free" is no statement)
    if (m.normal_explicit) s += "NX;";
    // Eliminate: the group's index space (such a file always runs on generated kernels)
    if (m.schur()) s += "S" + std::to_string(m.elim_space) + ";";
    // ReducedSystem("explicit"): the reduced system's form ("implicit" is no statement)
    if (m.schur() && m.reduced_explicit) s += "RX;";
    // LinearSolver("cholesky"): the Step's linear solver ("pcg" is no statement)
    if (m.direct_cholesky) s += "DC;";
    // RobustEnergy: per loss group its graph, kind and residual count (the scale is in the
    // templates' W leaf only by group, so kind and count are named here)
    for (auto& L : m.loss)
        s += "L" + std::to_string(L.graph) + ":" + (L.kind == gen::GLossGroup::Huber ? "huber" : "cauchy") + ":" +
             std::to_string(L.residuals.size()) + ";";
    *sig = s;
    if (use_pre) *use_pre = m.use_preconditioner;
    return true;
}

namespace {
// The energy each hand-written family implements: energies/<family>.t, embedded at build
// time (Makefile: build/gen/family_energies_src.h). Each lowers to exactly the reference
// example's templates (tests/test_generic_frontend.py).
const std::pair<const char*, const char*> kFamilyEnergies[] = {
#include "family_energies_src.h"
};
}  // namespace

bool family_is_canonical(ProblemSpec* spec, std::string* why) {
    static std::mutex mu;
    static std::map<std::string, std::string> canon;   // family -> signature
    std::lock_guard<std::mutex> lk(mu);
    if (!canon.count(spec->family)) {
        for (auto& fe : kFamilyEnergies) {
            if (spec->family != fe.first) continue;
            std::string sig, err;
            if (!generic_signature(fe.second, &sig, nullptr, &err)) {
                *why = "canonical energy of family " + spec->family + " does not lower: " + err;
                return false;
            }
            canon[spec->family] = sig;
        }
        if (!canon.count(spec->family)) { *why = "no canonical energy for family " + spec->family; return false; }
    }
    std::string sig, err;
    bool use_pre = false;
    if (!generic_signature(spec->text, &sig, &use_pre, &err)) {
        *why = err;
        return false;
    }
    if (sig != canon[spec->family]) {
        *why = "the energy's residuals differ from the " + spec->family + " family's";
        return false;
    }
    spec->use_preconditioner = use_pre;
    return true;
}

template <typename TT>
class GenericOp {
public:
    using T = TT;
    static constexpr const char* kName = "generic";
    static constexpr const char* kApplyName = "gen_apply";
    static constexpr bool kSlabs = true;   // decided per energy: slab_refusal()

    GenericOp(const ProblemSpec& spec, const StateOptions& opts, Domain dom) : opts_(opts), dom_(dom) {
        std::string err;
        if (!gen::build_model(spec.text, &m_, &err)) {
            fprintf(stderr, "[opt_amd] generic: %s\n", err.c_str());
            exit(1);
        }
        unk_ = m_.unknown_images();
        if (m_.block_preconditioner) groups_ = m_.block_groups();
        const gen::GImage& u0 = m_.images[unk_[0]];
        dims_[0] = dims_[1] = dims_[2] = 1;
        for (size_t k = 0; k < u0.dims.size(); ++k) dims_[k] = (int)spec.dim_values.at(m_.dims[u0.dims[k]].index);
        npix_ = (long long)dims_[0] * dims_[1] * dims_[2];
        own_lo_ = 0;
        own_hi_ = npix_;
        if (u0.dims.size() == 2) {   // a row slab (StencilPlan::set_decomposition) or the whole image
            npix_ = dom.npix_mem();
            ymem0_ = dom.y_mem0;
            own_lo_ = dom.off(0, dom.y_lo);
            own_hi_ = dom.off(0, dom.y_hi);
        }
        multi_ = m_.multi();
        if (multi_) {
            // several index spaces: per-space sizes; the flag bytes of the unknown-carrying
            // spaces concatenated in unknown order. No slabs (slab_refusal), so the Domain is
            // only the flat extent of the flags.
            for (size_t sp = 0; sp < m_.spaces.size() && sp < 8; ++sp) {
                sdims_[sp][0] = sdims_[sp][1] = sdims_[sp][2] = 1;
                snpix_[sp] = 1;
                for (size_t k = 0; k < m_.spaces[sp].size(); ++k) {
                    sdims_[sp][k] = (int)spec.dim_values.at(m_.dims[m_.spaces[sp][k]].index);
                    snpix_[sp] *= sdims_[sp][k];
                }
            }
            nflags_ = 0;
            npix_ = 0;
            for (int sp : m_.unknown_spaces()) {
                fbase_[sp] = nflags_;
                nflags_ += snpix_[sp];
                npix_ = std::max(npix_, snpix_[sp]);   // (the launch grid's extent)
            }
            ymem0_ = 0;
            own_lo_ = own_hi_ = 0;
        }
        halo_ = row_halo();
        for (size_t g = 0; g < m_.graphs.size(); ++g) {
            long long e = 1;
            for (int d : m_.graphs[g].dims) e *= spec.dim_values.at(m_.dims[d].index);
            nedge_[g] = (int)e;
        }
        long long off = 0;
        for (size_t k = 0; k < unk_.size(); ++k) {
            uoff_[k] = off;
            off += pixels_of(unk_[k]) * m_.images[unk_[k]].channels;
        }
        n_ = off;
        src_ = gen::generate(m_, sizeof(T) == 8, gather_offsets_fit_32(m_, spec, sizeof(T) == 8));
        load_module();
        for (size_t i = 0; i < m_.images.size(); ++i)
            if (m_.images[i].internal) {   // ComputedArray values and gradient images
                dimg_[i] = dmalloc(std::max<size_t>(1, image_bytes(i)));
                OPT_HIP_CHECK(hipMemset(dimg_[i], 0, image_bytes(i)));
                a_.img[i] = dimg_[i];
            }
        // RobustEnergy: the cached weights, one value per edge in edge order per group and one
        // per (group, slot) in that slot's incidence order (filled by gen_loss_weights)
        for (size_t g = 0; g < m_.loss.size(); ++g) {
            lwe_[g] = dmalloc(sizeof(T) * std::max(1, nedge_[m_.loss[g].graph]));
            a_.lwe[g] = lwe_[g];
        }
        for (size_t i = 0; i < src_.loss_inc.size() && i < 16; ++i) {
            lwq_[i] = dmalloc(sizeof(T) * std::max(1, nedge_[m_.loss[src_.loss_inc[i].first].graph]));
            a_.lwq[i] = lwq_[i];
        }
        if (opts_.host_buffers) {
            for (size_t i = 0; i < m_.images.size(); ++i)
                if (!m_.images[i].internal) dimg_[i] = dmalloc(std::max<size_t>(1, image_bytes(i)));
            int sb = 0;
            for (size_t g = 0; g < m_.graphs.size(); ++g)
                for (size_t s = 0; s < m_.graphs[g].slot_names.size(); ++s, ++sb)
                    dslot_[sb] = (int*)dmalloc(sizeof(int) * std::max(1, nedge_[g]));
        }
    }
    ~GenericOp() {
        for (void* p : dimg_) dfree(p);
        for (int* p : dslot_) dfree(p);
        for (int k = 0; k < 16; ++k) { dfree(goff_[k]); dfree(geid_[k]); }
        for (int k = 0; k < 32; ++k) dfree(gnb_[k]);
        for (void* p : lwe_) dfree(p);
        for (void* p : lwq_) dfree(p);
        for (int* p : lpos_) dfree(p);
        dfree(fp_scratch_);
        if (mod_) (void)hipModuleUnload(mod_);
    }

    VecLayout layout() const {
        VecLayout L{};
        L.nimg = (int)unk_.size();
        for (size_t k = 0; k < unk_.size(); ++k) {
            L.ch[k] = m_.images[unk_[k]].channels;
            L.off[k] = uoff_[k];
        }
        L.off[L.nimg] = n_;
        L.N = multi_ ? nflags_ : npix_;
        for (size_t k = 0; k < unk_.size() && multi_; ++k) L.fbase[k] = fbase_[m_.images[unk_[k]].space];
        return L;
    }
    int halo() const { return halo_; }
    // Why this energy cannot run on row slabs ("" = it can). Graph and sampled reads are
    // data-dependent (as the optical_flow / ARAP families), slabs split the 2nd dimension.
    std::string slab_refusal() const {
        // (a halo element's z needs its neighbours' blocks: a change of its own)
        if (m_.block_preconditioner)
            return "generic: no row-slab decomposition with the block preconditioner (UsePreconditioner(\"block\"))";
        if (multi_) return "generic: no row-slab decomposition for an energy over several index spaces";
        if (m_.unknown_dims() != 2) return "generic: row-slab decomposition needs a 2-D energy";
        if (!m_.graphs.empty()) return "generic: no row-slab decomposition for graph energies";
        // (sampled reads may sit in a residual or, cached per Step, in a ComputedArray)
        std::vector<int> roots;
        for (auto& r : m_.residuals) roots.push_back(r.expr);
        for (auto& c : m_.computed) {
            roots.insert(roots.end(), c.expr.begin(), c.expr.end());
            for (auto& g : c.grads) roots.push_back(g.expr);
        }
        for (int e : roots) {
            bool sample = false;
            m_.pool.visit(e, [&](int, const gen::Node& n) { sample |= n.op == gen::Op::Sample; });
            if (sample) return "generic: no row-slab decomposition with sampled images (data-dependent reads)";
        }
        return "";
    }
    int stencil_blocks() const {
        long long w = std::max(npix_, n_);
        if (multi_) w = npix_;   // every loop walks one space's elements (or a graph's edges)
        for (int e : nedge_) w = std::max<long long>(w, e);
        return (int)std::max<long long>(1, std::min<long long>((w + kBlock - 1) / kBlock, max_blocks_));
    }

    void bind(void** params, hipStream_t s) {
        user_ = params;
        for (size_t i = 0; i < m_.images.size(); ++i) {
            if (m_.images[i].internal) continue;
            void* p = params[m_.images[i].index];
            if (opts_.host_buffers) {
                OPT_HIP_CHECK(hipMemcpyAsync(dimg_[i], p, image_bytes(i), hipMemcpyHostToDevice, s));
                p = dimg_[i];
            }
            a_.img[i] = p;
        }
        // an Array on an Unknown's slot views the (device copy of the) unknown
        for (size_t i = 0; i < m_.images.size(); ++i)
            if (!m_.images[i].unknown && !m_.images[i].internal && m_.images[i].tvalued)
                for (int k : unk_)
                    if (m_.images[k].index == m_.images[i].index) a_.img[i] = a_.img[k];
        for (size_t j = 0; j < m_.params.size(); ++j) {
            const void* p = params[m_.params[j].index];
            const std::string& t = m_.params[j].type;
            a_.prm[j] = t == "double" ? *(const double*)p
                        : (t == "int" || t == "int32") ? (double)*(const int*)p
                        : t == "uint" || t == "uint32" ? (double)*(const unsigned*)p
                                                       : (double)*(const float*)p;
        }
        // a loss group's Param scale, as bound now (gen_loss_weights and gen_cost read it from prm)
        for (auto& L : m_.loss)
            if (L.scale_param >= 0 && !(a_.prm[L.scale_param] > 0.0))
                throw PlanError("generic: RobustEnergy: the scale Param '" + m_.params[L.scale_param].name + "' is " +
                                std::to_string(a_.prm[L.scale_param]) + " (a loss scale must be positive)");
        int sb = 0;
        for (size_t g = 0; g < m_.graphs.size(); ++g) {
            for (size_t k = 0; k < m_.graphs[g].slot_names.size(); ++k, ++sb) {
                const int* v = (const int*)params[m_.graphs[g].slot_index[k]];
                if (opts_.host_buffers) {
                    OPT_HIP_CHECK(hipMemcpyAsync(dslot_[sb], v, sizeof(int) * nedge_[g], hipMemcpyHostToDevice, s));
                    v = dslot_[sb];
                }
                a_.slot[sb] = v;
            }
            a_.nedge[g] = nedge_[g];
        }
        if (sb > 0) check_graphs(s);
        for (int k = 0; k < 3; ++k) a_.dims[k] = dims_[k];
        a_.npix = npix_;
        a_.ymem0 = ymem0_;
        a_.own_lo = own_lo_;
        a_.own_hi = own_hi_;
        for (size_t k = 0; k < unk_.size(); ++k) a_.uoff[k] = uoff_[k];
        for (size_t sp = 0; sp < m_.spaces.size() && sp < 8 && multi_; ++sp) {
            for (int k = 0; k < 3; ++k) a_.sdims[sp][k] = sdims_[sp][k];
            a_.snpix[sp] = snpix_[sp];
            a_.fbase[sp] = fbase_[sp];
        }
    }
    // hipGraph replay gate + key (StencilPlan::pcg_graph_begin), from the lowered model:
    // no capture for graph energies (adjacency rebuilt on bind); the key is the argument
    // block every captured launch receives — image / slot / incidence pointers and
    // parameter values as bound by bind().
    bool capture_key(std::vector<unsigned long long>* key) const {
        if (!m_.graphs.empty()) return false;
        unsigned long long w[(sizeof(GenArgs) + 7) / 8] = {};
        memcpy(w, &a_, sizeof(GenArgs));
        key->insert(key->end(), w, w + (sizeof(GenArgs) + 7) / 8);
        return true;
    }
    void unbind(hipStream_t s) {
        if (!opts_.host_buffers) return;
        for (int k : unk_)
            OPT_HIP_CHECK(hipMemcpyAsync(user_[m_.images[k].index], dimg_[k], image_bytes(k), hipMemcpyDeviceToHost, s));
    }
    T* unknown(int k) { return k < (int)unk_.size() ? (T*)a_.img[unk_[k]] : nullptr; }
    void precompute(hipStream_t s) {
        for (hipFunction_t f : k_pre_) launch(f, s, {&a_});
    }
    // The private caches of values derived from the bound arrays, from the arrays bound at
    // this Step (StencilPlan::step; HasRefreshCaches): the per-step sample caches among the
    // ComputedArrays' kernels (GComputed::per_step) and the transcendental caches (the
    // precompute kernels after the ComputedArrays' ones: the centred cache image, the graph
    // record cache). The energy's own ComputedArrays are not touched: they keep the
    // reference's schedule. Returns whether any ran.
    bool refresh_caches(hipStream_t s) {
        bool ran = false;
        for (size_t k = 0; k < k_pre_.size(); ++k)
            if (k >= m_.computed.size() || m_.computed[k].per_step) {
                launch(k_pre_[k], s, {&a_});
                ran = true;
            }
        return ran;
    }
    // ComputedArray values and gradient images: exchanged after every precompute
    void computed_planes(std::vector<HaloPlane>& v) const {
        for (size_t i = 0; i < m_.images.size(); ++i)
            if (m_.images[i].internal)
                v.push_back({dimg_[i], (size_t)elem_size(m_.images[i], sizeof(T) == 8) * m_.images[i].channels *
                                           (size_t)dims_[0]});
    }

    void jtf(T* r, T* diag, uint8_t* flags, hipStream_t s) {
        a_.flags = flags;
        if (m_.block_preconditioner) {   // the same kernels with the blocks' triangle beside diag
            launch(k_jtf_, s, {&a_, &r, &diag, &blk_});
            if (src_.has_graph) launch(k_jtf_graph_, s, {&a_, &r, &diag, &blk_});
            return;
        }
        launch(k_jtf_, s, {&a_, &r, &diag});   // flags, and r / diag of the centred residuals
        if (src_.has_graph) launch(k_jtf_graph_, s, {&a_, &r, &diag});
    }

    // ---- block preconditioner (UsePreconditioner("block"); StencilPlan: HasBlockPre) ----
    // The plan owns the buffers: blk (block_entries() values: every group's packed lower
    // triangles, entry index slowest) is filled by jtf next to diag, factored and inverted in
    // place by block_init, and read by the other kernels; z is PCG's z = M^-1 r.
    bool block_pre() const { return m_.block_preconditioner; }
    long long block_entries() const {
        long long n = 0;
        for (auto& g : groups_) n += (long long)g.entries() * pixels_of(g.images[0]);
        return n;
    }
    void set_block_buffer(T* blk) { blk_ = blk; }
    // per unknown image (VecLayout order): its group and the block row of its first channel
    int block_layout(int max_images, int* group, int* first_row) const {
        for (size_t k = 0; k < unk_.size() && (int)k < max_images; ++k)
            for (size_t g = 0; g < groups_.size(); ++g)
                for (size_t q = 0; q < groups_[g].images.size(); ++q)
                    if (groups_[g].images[q] == unk_[k]) {
                        if (group) group[k] = (int)g;
                        if (first_row) first_row[k] = groups_[g].first_row[q];
                    }
        return (int)groups_.size();
    }
    void block_init(const T* r, const T* pre, const T* ctc, T* z, T* p, int lm, ReduceSlot rs, hipStream_t s) {
        launch(k_blk_init_, s, {&a_, &r, &pre, &ctc, &blk_, &z, &p, &lm, &rs});
    }
    void block_step2(const T* p, const T* Ap, const T* b, T* r, T* delta, T* z, const double* sc, int i_num, int i_den,
                     int first, int lm, int dl, const int* stop, ReduceSlot rs, ZetaArgs zt, hipStream_t s) {
        launch(k_blk_step2_, s, {&a_, &p, &Ap, &blk_, &b, &r, &delta, &z, &sc, &i_num, &i_den, &first, &lm, &dl, &stop, &rs,
                                 &zt.q0, &zt.stop, &zt.liter, &zt.q_tol, &zt.on});
    }
    void block_half2(const T* Adelta, const T* b, const T* delta, T* r, T* z, const int* stop, ReduceSlot rs, ZetaArgs zt,
                     hipStream_t s) {
        launch(k_blk_half2_, s, {&a_, &Adelta, &b, &blk_, &delta, &r, &z, &stop, &rs, &zt.q0, &zt.stop, &zt.liter, &zt.q_tol,
                                 &zt.on});
    }
    void block_apply(const T* rin, T* zout, hipStream_t s) { launch(k_blk_apply_, s, {&a_, &blk_, &rin, &zout}); }

    // ---- Schur complement (Eliminate(X, ...); StencilPlan: HasSchur; gen/codegen_schur.cpp) ----
    // The plan owns two compact vectors of schur_entries() values (the eliminated images'
    // elements): w (M^-1-sized products) and the stash of b_e. schur_rhs inverts the eliminated
    // blocks in place (before block_init, which then skips them), stashes and clears b_e, leaves
    // w = M^-1 b_e and publishes 1/2 b_e.M^-1 b_e; schur_elim is w = -M^-1 E^T p, or with the
    // stash the back-substitution into the full vector `out`; schur_apply is Ap = B p + E w.
    bool schur() const { return m_.schur(); }
    long long schur_entries() const {
        long long n = 0;
        for (int k : m_.eliminated) n += pixels_of(k) * m_.images[k].channels;
        return n;
    }
    void set_schur_buffers(T* w, T* be) { w_ = w; be_ = be; }
    // per unknown image (VecLayout order): 1 if eliminated
    int eliminated(int max_images, int* flag) const {
        for (size_t k = 0; k < unk_.size() && (int)k < max_images; ++k)
            if (flag) flag[k] = m_.is_eliminated(unk_[k]) ? 1 : 0;
        return (int)unk_.size();
    }
    void schur_rhs(const T* ctc, T* r, T* b, int lm, ReduceSlot rs, hipStream_t s) {
        launch(k_schur_rhs_, s, {&a_, &blk_, &ctc, &r, &b, &be_, &w_, &lm, &rs});
    }
    void schur_elim(const T* p, hipStream_t s) {
        const T* rhs = nullptr;
        int full = 0;
        launch(k_schur_elim_, s, {&a_, &blk_, &p, &rhs, &w_, &full});
    }
    void schur_back(T* delta, hipStream_t s) {
        const T* p = delta;
        int full = 1;
        launch(k_schur_elim_, s, {&a_, &blk_, &p, &be_, &delta, &full});
    }
    void schur_apply(const T* p, T* Ap, const T* dadd, const int* stop, ReduceSlot rs, hipStream_t s) {
        launch(k_schur_apply_, s, {&a_, &p, &w_, &Ap, &dadd, &stop, &rs});
    }
    // ---- the assembled matrix (ReducedSystem("explicit"): S; NormalMatrix("explicit"): H = J^T J;
    // StencilPlan: HasExplicitMatrix; explicit_matrix.h; gen/codegen_schur_explicit.cpp, codegen_normal.cpp) ----
    // A file has at most one of the two statements: matrix_form() says which. Symbolic phase:
    // block-CSR pattern, per-block pair lists and the long blocks / rows, built from the vertex
    // arrays at the first use and again when the graphs were re-wired. Numeric phase, once per
    // Step before block_init inverts the retained blocks in place — for S after schur_rhs (M_e^-1
    // in blk), for H after jtf (the diagonal blocks in blk): matrix_eblk writes W_q, Y_q (S) or
    // G_q (H) per edge instance, matrix_assemble sums the blocks. matrix_spmv then is
    // gen_schur_apply's / apply's contract on the assembled matrix.
    MatrixForm matrix_form() const {
        return src_.has_schur_explicit ? MatrixForm::Schur : src_.has_normal ? MatrixForm::Normal : MatrixForm::None;
    }
    bool matrix_symbolic_stale() const { return xm_.stale(topology_generation_); }
    void matrix_symbolic(hipStream_t s) {
        if (!matrix_symbolic_stale()) return;
        std::vector<SchurListDev> lists;
        if (src_.has_schur_explicit) {   // the lists in the eliminated slots' incidence order
            if (src_.schur_lists.size() > 16) throw PlanError("generic: ReducedSystem(\"explicit\"): more than 16 instance lists");
            for (auto& l : src_.schur_lists)
                lists.push_back({a_.slot[l.eslot], a_.slot[l.rslot], geid_[l.eslot], nedge_[l.graph], 0});
            xm_.build({"explicit Schur complement", false, src_.schur_cr, src_.schur_cr * src_.schur_ce, 2, 0},
                      snpix_[m_.elim_space], snpix_[src_.schur_rspace], lists, topology_generation_, s);
            return;
        }
        if (src_.normal_lists.size() > 16) throw PlanError("generic: NormalMatrix(\"explicit\"): more than 16 instance lists");
        // the edges of the graphs with lists, numbered graph after graph: edge e of graph g is
        // "eliminated vertex" ebase[g] + e, and its instance in a list sits at position e (the
        // edge is the vertex, the order the identity)
        long long ebase[4] = {0, 0, 0, 0}, ne = 0;
        for (size_t g = 0; g < m_.graphs.size() && g < 4; ++g) {
            bool used = false;
            for (auto& l : src_.normal_lists) used |= l.graph == (int)g;
            ebase[g] = ne;
            if (used) ne += nedge_[g];
        }
        for (auto& l : src_.normal_lists) lists.push_back({nullptr, a_.slot[l.slot], nullptr, nedge_[l.graph], ebase[l.graph]});
        xm_.build({"NormalMatrix(\"explicit\")", true, src_.normal_c, src_.normal_c * src_.normal_r, 1, gen::kNormalLongRow},
                  ne, pixels_of(groups_[0].images[0]), lists, topology_generation_, s);
    }
    void matrix_eblk(hipStream_t s) {
        const auto& m = xm_.buffers();
        if (src_.has_normal) launch(k_mx_eblk_, s, {&a_, &m.inst[0], &m.qbase});
        else launch(k_mx_eblk_, s, {&a_, &blk_, &m.inst[0], &m.inst[1], &m.qbase});
    }
    void matrix_assemble(hipStream_t s) {
        const auto& m = xm_.buffers();
        // blocks per workgroup: 4, in H's packed form 4 per 64 / C^2 lanes; H's kernels take G_q as W_q and Y_q
        const long long per_wg = src_.has_normal ? 4 * (64 / (src_.normal_c * src_.normal_c)) : 4;
        T* const* yq = src_.has_normal ? &m.inst[0] : &m.inst[1];
        const int nnzb = (int)m.nnzb;
        const int grid = (int)std::max<long long>(1, std::min<long long>((m.nnzb + per_wg - 1) / per_wg, 1 << 18));
        launch_grid(k_mx_assemble_, grid, s, {&a_, &blk_, &m.inst[0], yq, &m.blkRow, &m.colInd, &m.pairPtr, &m.pairs, &m.val, &nnzb});
        if (m.nLong > 0)
            launch_grid(k_mx_assemble_long_, std::min(m.nLong, 1 << 16), s,
                        {&a_, &blk_, &m.inst[0], yq, &m.blkRow, &m.colInd, &m.pairPtr, &m.pairs, &m.val, &m.longBlk, &m.nLong});
    }
    void matrix_spmv(const T* p, T* Ap, const T* dadd, const int* stop, ReduceSlot rs, hipStream_t s) {
        const auto& m = xm_.buffers();
        if (src_.has_normal) launch(k_mx_spmv_, s, {&a_, &m.rowPtr, &m.colInd, &m.val, &p, &Ap, &dadd, &stop, &rs, &m.longRow, &m.nLongRow});
        else launch(k_mx_spmv_, s, {&a_, &m.rowPtr, &m.colInd, &m.val, &p, &Ap, &dadd, &stop, &rs});
    }
    bool matrix_shape(long long* rows, int* dim, long long* nnzb) const { return xm_.shape(rows, dim, nnzb); }
    void matrix_copy(int* rowPtr, int* colInd, T* val, hipStream_t s) { xm_.copy_out(rowPtr, colInd, val, s); }
    void matrix_key(std::vector<unsigned long long>* key) const { xm_.capture_key(key); }
    const std::string& symbolic_info() const { return xm_.info(); }
    // ---- LinearSolver("cholesky") (StencilPlan: direct_step; gen/codegen_dense.cpp) ----
    // dense_fill: the assembled matrix plus dadd into the zeroed tiles of a DenseFactor, the
    // original diagonal and the right-hand side from r; dense_store: the solution into delta.
    bool direct_solver() const { return src_.has_dense; }
    void dense_fill(const T* dadd, const T* r, T* tiles, T* diag0, T* rhs, hipStream_t s) {
        const auto& m = xm_.buffers();
        const long long nnzb = m.nnzb;
        const int grid = (int)std::max<long long>(1, std::min<long long>(nnzb, 1 << 20));
        launch_grid(k_dense_fill_, grid, s, {&a_, &m.blkRow, &m.colInd, &m.val, &nnzb, &dadd, &r, &tiles, &diag0, &rhs});
    }
    void dense_store(const T* x, T* delta, const int* fail, hipStream_t s) {
        launch(k_dense_store_, s, {&a_, &x, &delta, &fail});
    }
    // ---- robust losses (RobustEnergy; StencilPlan: HasLossWeights; gen/codegen.cpp emit_loss_weights) ----
    // loss_weights caches w = sqrt(rho'(s)) per edge for the kernels of this linearisation: after
    // every precompute (Init, update, revert, the stand-alone entry points) and at Step start,
    // after the caches its residuals may read. eval_loss_rho1 writes rho'(s) of one group to the
    // caller's array and leaves the caches alone.
    bool has_loss() const { return src_.has_loss; }
    void loss_weights(hipStream_t s) {
        T* none = nullptr;
        int all = -1;
        launch(k_loss_weights_, s, {&a_, &none, &all});
    }
    int loss_groups(int max_groups, int* graph, int* residuals, int* kind) const {
        for (size_t g = 0; g < m_.loss.size() && (int)g < max_groups; ++g) {
            if (graph) graph[g] = m_.loss[g].graph;
            if (residuals) residuals[g] = (int)m_.loss[g].residuals.size();
            if (kind) kind[g] = m_.loss[g].kind;
        }
        return (int)m_.loss.size();
    }
    long long loss_group_edges(int group) const {
        return group >= 0 && group < (int)m_.loss.size() ? nedge_[m_.loss[group].graph] : -1;
    }
    void eval_loss_rho1(int group, T* out, hipStream_t s) {
        if (group < 0 || group >= (int)m_.loss.size())
            throw PlanError("generic: OptAMD_EvalLossWeights: loss group " + std::to_string(group) + " of " +
                            std::to_string(m_.loss.size()));
        T* dst = out;
        const size_t bytes = sizeof(T) * (size_t)nedge_[m_.loss[group].graph];
        if (opts_.host_buffers) dst = (T*)dmalloc(std::max<size_t>(1, bytes));
        launch(k_loss_weights_, s, {&a_, &dst, &group});
        if (opts_.host_buffers) {
            OPT_HIP_CHECK(hipMemcpyAsync(out, dst, bytes, hipMemcpyDeviceToHost, s));
            OPT_HIP_CHECK(hipStreamSynchronize(s));
            dfree(dst);
        }
    }
    void apply(const T* p, T* Ap, const T* dadd, const int* stop, ReduceSlot rs, hipStream_t s) {
        if (!src_.has_graph) {
            int finish = 1;
            launch(k_apply_, s, {&a_, &p, &Ap, &dadd, &stop, &rs, &finish});
            return;
        }
        int finish = 0, centred = src_.has_centered && !src_.graph_apply_centred ? 1 : 0;
        if (centred) launch(k_apply_, s, {&a_, &p, &Ap, &dadd, &stop, &rs, &finish});
        launch(k_apply_graph_, s, {&a_, &p, &Ap, &dadd, &stop, &rs, &centred});
    }
    void cost(ReduceSlot rs, hipStream_t s) {
        const T* d = nullptr;
        launch(k_cost_, s, {&a_, &d, &rs});
    }
    void model_cost(const T* delta, ReduceSlot rs, hipStream_t s) { launch(k_cost_, s, {&a_, &delta, &rs}); }

    // materialized Jacobian (useMaterializedJTJ, csr.h): the generated saveJToCRS kernels
    // (none over several index spaces: -1, and dump_j refuses)
    long long jacobian_rows() const {
        if (multi_ || src_.has_loss) return -1;
        long long r = 0;
        for (auto& d : src_.dump) r += elements(d.graph) * d.rows;
        return r;
    }
    long long jacobian_nnz() const {
        if (multi_ || src_.has_loss) return -1;
        long long z = 0;
        for (auto& d : src_.dump) z += elements(d.graph) * d.nnz;
        return z;
    }
    void dump_j(int* rowPtr, int* colInd, T* val, hipStream_t s) {
        if (src_.has_loss) throw PlanError("generic: no Jacobian assembly (OptAMD_EvalJacobian) for an energy with a RobustEnergy statement");
        if (multi_) throw PlanError("generic: no Jacobian assembly (OptAMD_EvalJacobian) for an energy over several index spaces");
        long long rb = 0, zb = 0;
        for (size_t i = 0; i < src_.dump.size(); ++i) {
            launch(k_dump_[i], s, {&a_, &rowPtr, &colInd, &val, &rb, &zb, &n_});
            rb += elements(src_.dump[i].graph) * src_.dump[i].rows;
            zb += elements(src_.dump[i].graph) * src_.dump[i].nnz;
        }
        OPT_HIP_CHECK(hipMemsetD32Async(rowPtr + rb, (int)zb, 1, s));
    }
    // the graphs' vertex arrays changed (check_graphs; stencil_plan.h, HasTopologyGeneration)
    unsigned long long topology_generation() const { return topology_generation_; }

    // The forms load_module chose (OptAMD_PlanGeneratedForms; StencilPlan: HasGeneratedForms), the
    // grid every generated kernel is launched with, and per strip form the rows a wave walks:
    // the strips' own rule (codegen_strip.cpp open_waves) for this grid of 4-wave blocks.
    std::string generated_forms() const {
        const int grid = stencil_blocks(), H = dims_[1];
        auto row_block = [&](const char* form, int cols) {
            if (std::string(form) != "strip") return 0;
            const long long nsx = (dims_[0] + cols - 1) / cols, G = 4LL * grid;
            return (int)std::max<long long>(8, ((long long)H * nsx + G - 1) / G);
        };
        char line[256];
        snprintf(line, sizeof line, "apply=%s jtf=%s cost=%s grid=%d rows=%d apply_row_block=%d jtf_row_block=%d cost_row_block=%d",
                 apply_form_, jtf_form_, cost_form_, grid, H, row_block(apply_form_, src_.strip_cols),
                 row_block(jtf_form_, src_.jtf_strip_cols), row_block(cost_form_, src_.cost_strip_cols));
        return line;
    }

    const std::string& source() const { return src_.code; }
    bool tiled_selected() const { return k_apply_ == k_apply_tiled_; }

private:
    long long elements(int graph) const { return graph < 0 ? npix_ : nedge_[graph]; }
    // Rows a slab must hold beyond its own: the widest vertical reach of any residual
    // instance that touches an owned unknown (the span of its reads incl. ComputedArray
    // boxes), of the ComputedArrays' own expressions, and of the exclusion test.
    int row_halo() const {
        if (m_.unknown_dims() != 2) return 0;
        auto reach = [&](int e, int* lo, int* hi) {
            m_.pool.visit(e, [&](int, const gen::Node& n) {
                if (n.op != gen::Op::Read || n.slot >= 0) return;
                int clo = 0, chi = 0;
                for (auto& c : m_.computed)
                    if (c.image == n.i) { clo = c.lo[1]; chi = c.hi[1]; }
                *lo = std::min(*lo, n.off[1] + clo);
                *hi = std::max(*hi, n.off[1] + chi);
            });
        };
        int h = 0;
        for (auto& r : m_.residuals) {
            int lo = 0, hi = 0;
            reach(r.expr, &lo, &hi);
            h = std::max(h, hi - lo);
        }
        for (auto& c : m_.computed) h = std::max({h, -c.lo[1], c.hi[1]});
        if (m_.exclude >= 0) {
            int lo = 0, hi = 0;
            reach(m_.exclude, &lo, &hi);
            h = std::max({h, -lo, hi});
        }
        return std::max(h, 1);
    }
    size_t image_bytes(size_t i) const {
        return (size_t)pixels_of(i) * m_.images[i].channels * elem_size(m_.images[i], sizeof(T) == 8);
    }
    // elements of image i: its own index space's
    long long pixels_of(size_t i) const { return multi_ ? snpix_[m_.images[i].space] : npix_; }
    // elements of the space graph g's slot k indexes
    long long slot_pixels(size_t g, size_t k) const { return multi_ ? snpix_[m_.graphs[g].slot_space[k]] : npix_; }
    void load_module() {
        std::string obj;
        {
            std::lock_guard<std::mutex> lk(g_mu);
            auto it = code_cache().find(src_.code);
            if (it != code_cache().end()) obj = it->second;
        }
        if (obj.empty()) {
            std::string log;
            if (!rtc_compile(src_.code, &obj, &log)) {
                fprintf(stderr, "[opt_amd] generic: generated kernels failed to compile:\n%s\n", log.c_str());
                exit(1);
            }
            std::lock_guard<std::mutex> lk(g_mu);
            code_cache()[src_.code] = obj;
        }
        OPT_HIP_CHECK(hipModuleLoadData(&mod_, obj.data()));
        for (auto kv : {std::make_pair(&k_jtf_, "gen_jtf"), std::make_pair(&k_apply_, "gen_apply"),
                        std::make_pair(&k_cost_, "gen_cost"), std::make_pair(&k_jtf_graph_, "gen_jtf_graph"),
                        std::make_pair(&k_apply_graph_, "gen_apply_graph")})
            OPT_HIP_CHECK(hipModuleGetFunction(kv.first, mod_, kv.second));
        // Centred apply: the register strip where the front end emitted one, else the
        // two-phase LDS tiles where it prefers them (prefer_tiled: many residual instances
        // per pixel), else the gather. OPT_AMD_GEN_APPLY=gather|tiled|strip forces one.
        // (Row slabs use the gather: its reads stay within row_halo() of the owned rows.)
        const bool slab = dom_.mem_rows != dom_.H || dom_.y_lo != 0;
        const char* want = getenv("OPT_AMD_GEN_APPLY");
        const std::string force = want ? want : "";
        if (src_.has_tiled && !slab) {
            OPT_HIP_CHECK(hipModuleGetFunction(&k_apply_tiled_, mod_, "gen_apply_tiled"));
            if (force == "tiled" || (force.empty() && src_.prefer_tiled)) { k_apply_ = k_apply_tiled_; apply_form_ = "tiled"; }
        }
        if (src_.has_strip && !slab) {
            // one wave per (column strip, >= 8-row block): a small image leaves most SIMDs
            // idle (poisson 512^2: 576 waves, 13.7 -> 20.4 us), so below ~2 waves per SIMD
            // the other forms run
            OPT_HIP_CHECK(hipModuleGetFunction(&k_apply_strip_, mod_, "gen_apply_strip"));
            const long long waves = (long long)((dims_[0] + src_.strip_cols - 1) / src_.strip_cols) * ((dims_[1] + 7) / 8);
            if (force == "strip" || (force.empty() && waves >= 2048)) { k_apply_ = k_apply_strip_; apply_form_ = "strip"; }
        }
        // Strip waves walk whole row blocks, so a grid of 1.33 resident rounds leaves a third
        // of the chip idle in its tail: with the strip apply, launch exactly the blocks that
        // are resident together (its occupancy x CUs; image_warping / shape_from_shading at
        // 80 VGPRs: 1536 blocks; measured 2048 -> 1536: generated image_warping apply
        // 228 -> 204 us, shape_from_shading LM step 4.18 -> 3.82 ms)
        if (k_apply_strip_ && k_apply_ == k_apply_strip_ && !getenv("OPT_AMD_GEN_BLOCKS")) {
            int per_cu = 0, dev = 0, cus = 0;
            OPT_HIP_CHECK(hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_apply_strip_, kBlock, 0));
            OPT_HIP_CHECK(hipGetDevice(&dev));
            OPT_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
            if (per_cu > 0 && cus > 0) max_blocks_ = std::min(4096, std::max(8, per_cu * cus));
        }
        // J^T F: the register strip under the same rule (OPT_AMD_GEN_JTF=gather|strip forces)
        if (m_.block_preconditioner) {
            for (auto kv : {std::make_pair(&k_blk_init_, "gen_blk_init"), std::make_pair(&k_blk_step2_, "gen_blk_step2"),
                            std::make_pair(&k_blk_half2_, "gen_blk_half2"), std::make_pair(&k_blk_apply_, "gen_blk_apply")})
                OPT_HIP_CHECK(hipModuleGetFunction(kv.first, mod_, kv.second));
        }
        if (src_.has_schur) {
            for (auto kv : {std::make_pair(&k_schur_rhs_, "gen_schur_rhs"), std::make_pair(&k_schur_elim_, "gen_schur_elim"),
                            std::make_pair(&k_schur_apply_, "gen_schur_apply")})
                OPT_HIP_CHECK(hipModuleGetFunction(kv.first, mod_, kv.second));
        }
        if (matrix_form() != MatrixForm::None) {   // gen_schur_eblk ... or gen_normal_eblk ...
            const std::string prefix = src_.has_normal ? "gen_normal_" : "gen_schur_";
            for (auto kv : {std::make_pair(&k_mx_eblk_, "eblk"), std::make_pair(&k_mx_assemble_, "assemble"),
                            std::make_pair(&k_mx_assemble_long_, "assemble_long"), std::make_pair(&k_mx_spmv_, "spmv")})
                OPT_HIP_CHECK(hipModuleGetFunction(kv.first, mod_, (prefix + kv.second).c_str()));
        }
        if (src_.has_dense) {
            OPT_HIP_CHECK(hipModuleGetFunction(&k_dense_fill_, mod_, "gen_dense_fill"));
            OPT_HIP_CHECK(hipModuleGetFunction(&k_dense_store_, mod_, "gen_dense_store"));
        }
        if (src_.has_loss) OPT_HIP_CHECK(hipModuleGetFunction(&k_loss_weights_, mod_, "gen_loss_weights"));
        // (the strip J^T F has no block accumulation: block energies keep the gather)
        if (src_.has_jtf_strip && !slab && !m_.block_preconditioner) {
            const char* wj = getenv("OPT_AMD_GEN_JTF");
            const std::string fj = wj ? wj : "";
            const long long waves = (long long)((dims_[0] + src_.jtf_strip_cols - 1) / src_.jtf_strip_cols) * ((dims_[1] + 7) / 8);
            if (fj == "strip" || (fj.empty() && waves >= 2048)) {
                OPT_HIP_CHECK(hipModuleGetFunction(&k_jtf_, mod_, "gen_jtf_strip"));
                jtf_form_ = "strip";
            }
        }
        // cost / model cost: the register strip under the same rule (OPT_AMD_GEN_COST forces)
        if (src_.has_cost_strip && !slab) {
            const char* wc = getenv("OPT_AMD_GEN_COST");
            const std::string fc = wc ? wc : "";
            const long long waves = (long long)((dims_[0] + src_.cost_strip_cols - 1) / src_.cost_strip_cols) * ((dims_[1] + 7) / 8);
            if (fc == "strip" || (fc.empty() && waves >= 2048)) {
                OPT_HIP_CHECK(hipModuleGetFunction(&k_cost_, mod_, "gen_cost_strip"));
                cost_form_ = "strip";
            }
        }
        k_dump_.resize(src_.dump.size());
        for (size_t k = 0; k < src_.dump.size(); ++k)
            OPT_HIP_CHECK(hipModuleGetFunction(&k_dump_[k], mod_, ("gen_dump_j_" + std::to_string(k)).c_str()));
        k_pre_.resize(src_.n_precompute);
        for (int k = 0; k < src_.n_precompute; ++k)
            OPT_HIP_CHECK(hipModuleGetFunction(&k_pre_[k], mod_, ("gen_precompute_" + std::to_string(k)).c_str()));
    }
    void launch(hipFunction_t f, hipStream_t s, std::initializer_list<const void*> args) {
        launch_grid(f, stencil_blocks(), s, args);
    }
    void launch_grid(hipFunction_t f, int grid, hipStream_t s, std::initializer_list<const void*> args) {
        std::vector<void*> a;
        for (const void* p : args) a.push_back(const_cast<void*>(p));
        OPT_HIP_CHECK(hipModuleLaunchKernel(f, grid, 1, 1, kBlock, 1, 1, 0, s, a.data(), nullptr));
    }
    // vertex indices must lie in [0, N) (fail-stop, as the reference does on bad input)
    void check_graphs(hipStream_t s) {
        if (!fp_scratch_)
            fp_scratch_ = (unsigned long long*)dmalloc(sizeof(unsigned long long) * (1 + kFingerprintGrid));
        int sb = 0;
        for (size_t g = 0; g < m_.graphs.size(); ++g) {
            const int ns = (int)m_.graphs[g].slot_names.size();
            const unsigned long long h = graph_fingerprint(a_.slot + sb, ns, nedge_[g], s, fp_scratch_);
            if (!(goff_[sb] && h == fingerprint_[g])) {
                // every slot against its own space, before any list is built or the
                // fingerprint kept: a bad index stops the solve (PlanError), no kernel reads it
                for (int k = 0; k < ns && nedge_[g] > 0; ++k) {
                    std::vector<int> hv(nedge_[g]);
                    OPT_HIP_CHECK(hipMemcpyAsync(hv.data(), a_.slot[sb + k], sizeof(int) * nedge_[g],
                                                 hipMemcpyDeviceToHost, s));
                    OPT_HIP_CHECK(hipStreamSynchronize(s));
                    const long long nv = slot_pixels(g, k);
                    for (int v : hv)
                        if (v < 0 || v >= nv) {
                            fingerprint_[g] = 0;
                            dfree(goff_[sb]);
                            goff_[sb] = nullptr;
                            throw PlanError("generic: graph '" + m_.graphs[g].name + "' slot '" +
                                            m_.graphs[g].slot_names[k] + "': vertex index " + std::to_string(v) +
                                            " outside [0, " + std::to_string(nv) + ")");
                        }
                }
                fingerprint_[g] = h;
                ++topology_generation_;
                for (int k = 0; k < ns; ++k) build_incidence(sb + k, nedge_[g], slot_pixels(g, k), s);
                for (int k = 0; k < ns; ++k) build_neighbours(sb + k, nedge_[g], s);
            }
            sb += ns;
        }
        for (int k = 0; k < sb; ++k) {
            a_.goff[k] = goff_[k];
            a_.geid[k] = geid_[k];
        }
        for (size_t i = 0; i < src_.nb_pairs.size() && i < 32; ++i) a_.gnb[i] = gnb_[i];
        for (int k = 0; k < sb && k < 16; ++k) a_.lpos[k] = lpos_[k];
    }
    // GenArgs::gnb of every (slot k, other slot) pair whose incidence list was rebuilt:
    // the other slot's vertex of each incident edge, in the incidence order
    void build_neighbours(int sb, int E, hipStream_t s) {
        for (size_t i = 0; i < src_.nb_pairs.size() && i < 32; ++i) {
            if (src_.nb_pairs[i].first != sb) continue;
            dfree(gnb_[i]);
            gnb_[i] = (int*)dmalloc(sizeof(int) * std::max(E, 1));
            if (E == 0) continue;
            const int grid = std::min((E + 255) / 256, 4096);
            hipLaunchKernelGGL(incidence_gather, dim3(grid), dim3(256), 0, s, a_.slot[src_.nb_pairs[i].second],
                               (const int*)geid_[sb], E, gnb_[i]);
            OPT_HIP_CHECK(hipGetLastError());
        }
    }
    // Edges by vertex for slot array sb: a stable radix sort of (vertex, edge id) pairs and
    // a histogram + exclusive scan of the vertex counts.
    void build_incidence(int sb, int E, long long nv, hipStream_t s) {
        dfree(goff_[sb]);
        dfree(geid_[sb]);
        goff_[sb] = (int*)dmalloc(sizeof(int) * (nv + 1));
        geid_[sb] = (int*)dmalloc(sizeof(int) * std::max(E, 1));
        OPT_HIP_CHECK(hipMemsetAsync(goff_[sb], 0, sizeof(int) * (nv + 1), s));
        if (E == 0) return;
        int* keys = (int*)dmalloc(sizeof(int) * E);
        int* ids = (int*)dmalloc(sizeof(int) * E);
        const int grid = std::min((E + 255) / 256, 4096);
        hipLaunchKernelGGL(iota_kernel, dim3(grid), dim3(256), 0, s, ids, E);
        int bits = 1;
        while ((1LL << bits) < nv) ++bits;
        size_t need = 0, need2 = 0;
        OPT_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, need, a_.slot[sb], keys, ids, geid_[sb], E, 0, bits, s));
        OPT_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, need2, goff_[sb], goff_[sb], (int)nv + 1, s));
        need = std::max(need, need2);
        void* tmp = dmalloc(std::max<size_t>(need, 1));
        OPT_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp, need, a_.slot[sb], keys, ids, geid_[sb], E, 0, bits, s));
        hipLaunchKernelGGL(incidence_count, dim3(grid), dim3(256), 0, s, a_.slot[sb], E, goff_[sb]);
        size_t n2 = need;
        OPT_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, n2, goff_[sb], goff_[sb], (int)nv + 1, s));
        // RobustEnergy: the inverse of geid for the slots that carry a group's unknowns
        for (auto& li : src_.loss_inc)
            if (li.second == sb && !lpos_[sb]) lpos_[sb] = (int*)dmalloc(sizeof(int) * E);
        if (lpos_[sb]) {
            hipLaunchKernelGGL(incidence_positions, dim3(grid), dim3(256), 0, s, (const int*)geid_[sb], E, lpos_[sb]);
            OPT_HIP_CHECK(hipGetLastError());
        }
        OPT_HIP_CHECK(hipStreamSynchronize(s));
        dfree(tmp);
        dfree(keys);
        dfree(ids);
    }

    StateOptions opts_;
    Domain dom_;
    int ymem0_ = 0, halo_ = 0;
    long long own_lo_ = 0, own_hi_ = 0;
    gen::GModel m_;
    gen::GenSource src_;
    std::vector<int> unk_;
    int dims_[3];
    long long npix_ = 0, n_ = 0;
    // several index spaces (GModel::spaces): sizes, flag bases, flag bytes in all
    bool multi_ = false;
    int sdims_[8][3] = {};
    long long snpix_[8] = {}, fbase_[8] = {}, nflags_ = 0;
    long long uoff_[4] = {0, 0, 0, 0};
    std::vector<int> nedge_ = std::vector<int>(4, 0);
    GenArgs a_{};
    void** user_ = nullptr;
    void* dimg_[16] = {};
    int* dslot_[16] = {};
    unsigned long long fingerprint_[4] = {0, 0, 0, 0};
    unsigned long long topology_generation_ = 0;   // bumped with every rebuild of the incidence lists
    unsigned long long* fp_scratch_ = nullptr;
    int* goff_[16] = {};
    int* geid_[16] = {};
    int* gnb_[32] = {};
    // RobustEnergy: weights in edge order per group, in incidence order per GenSource::loss_inc
    // entry, and per slot the inverse of geid (rebuilt with it)
    void* lwe_[4] = {};
    void* lwq_[16] = {};
    int* lpos_[16] = {};
    hipFunction_t k_loss_weights_{};
    // grid of every generic kernel (all walk their work grid-stride); a register-strip apply
    // sets it to the blocks the chip holds at once (below), OPT_AMD_GEN_BLOCKS overrides
    int max_blocks_ = std::min(4096, std::max(8, env_int("OPT_AMD_GEN_BLOCKS", 2048)));
    hipModule_t mod_ = nullptr;
    std::vector<hipFunction_t> k_pre_, k_dump_;
    hipFunction_t k_apply_tiled_{}, k_apply_strip_{};
    const char *apply_form_ = "gather", *jtf_form_ = "gather", *cost_form_ = "gather";   // what load_module chose
    hipFunction_t k_jtf_{}, k_apply_{}, k_cost_{}, k_jtf_graph_{}, k_apply_graph_{};
    hipFunction_t k_blk_init_{}, k_blk_step2_{}, k_blk_half2_{}, k_blk_apply_{};
    std::vector<gen::GBlockGroup> groups_;   // block preconditioner: empty without it
    T* blk_ = nullptr;                       // the plan's block buffer (set_block_buffer)
    hipFunction_t k_schur_rhs_{}, k_schur_elim_{}, k_schur_apply_{};
    T *w_ = nullptr, *be_ = nullptr;         // the plan's compact Schur vectors (set_schur_buffers)
    // the assembled S or H (matrix_form()): its eblk / assemble / SpMV kernels and its buffers
    hipFunction_t k_mx_eblk_{}, k_mx_assemble_{}, k_mx_assemble_long_{}, k_mx_spmv_{};
    hipFunction_t k_dense_fill_{}, k_dense_store_{};
    ExplicitMatrix<T> xm_;
};

static_assert(HasBlockPre<GenericOp<float>>::value);   // the optional driver features this Op claims (stencil_plan.h)
static_assert(HasSchur<GenericOp<float>>::value);
static_assert(HasExplicitMatrix<GenericOp<float>>::value);
static_assert(HasLossWeights<GenericOp<float>>::value);
static_assert(HasCaptureKey<GenericOp<float>>::value);
static_assert(HasRefreshCaches<GenericOp<float>>::value);
static_assert(HasSlabRefusal<GenericOp<float>>::value);
static_assert(HasTopologyGeneration<GenericOp<float>>::value);
static_assert(HasDumpJ<GenericOp<float>>::value);
static_assert(HasGeneratedForms<GenericOp<float>>::value);

std::unique_ptr<Plan> make_generic_plan(const ProblemSpec& spec, const StateOptions& opts, const unsigned* dims,
                                        std::string* err) {
    ProblemSpec s = spec;
    gen::GModel m;
    if (!gen::build_model(spec.text, &m, err)) return nullptr;
    int maxidx = -1;
    for (auto& d : m.dims) maxidx = std::max(maxidx, d.index);
    s.dim_values.assign(dims, dims + maxidx + 1);
    const std::vector<int>& ud = m.images[m.unknown_images()[0]].dims;
    auto pixels = [&](const std::vector<int>& dims) {
        long long n = 1;
        for (int d : dims) n *= s.dim_values[m.dims[d].index];
        return n;
    };
    // every declared space (one: the unknowns'), then the flag bytes of the unknown-carrying ones
    const long long npix = pixels(ud);
    for (auto& sp : m.spaces)
        if (pixels(sp) <= 0 || pixels(sp) > (1LL << 31) / 16) {
            *err = m.multi() ? "generic: index space empty or too large" : "generic: unknown index space empty or too large";
            return nullptr;
        }
    long long nflags = 0;
    if (m.schur() && (opts.materialized || opts.fused_jtj)) {
        *err = "generic: no materialized Jacobian (useMaterializedJTJ / useFusedJTJ) with Eliminate: the Schur "
               "complement runs matrix-free";
        return nullptr;
    }
    {
        const std::string why = gen::explicit_refusal(m);
        if (!why.empty()) { *err = "generic: " + why; return nullptr; }
    }
    {
        const std::string why = gen::normal_refusal(m);
        if (!why.empty()) { *err = "generic: " + why; return nullptr; }
    }
    if (m.normal_explicit && (opts.materialized || opts.fused_jtj)) {
        *err = "generic: no materialized Jacobian (useMaterializedJTJ / useFusedJTJ) with NormalMatrix(\"explicit\"): "
               "the plan forms J^T J itself";
        return nullptr;
    }
    if (!m.loss.empty() && (opts.materialized || opts.fused_jtj)) {
        *err = "generic: no materialized Jacobian (useMaterializedJTJ / useFusedJTJ) with RobustEnergy: the weights "
               "are the matrix-free kernels'";
        return nullptr;
    }
    if (m.multi()) {
        if (opts.materialized || opts.fused_jtj) {
            *err = "generic: no materialized Jacobian (useMaterializedJTJ / useFusedJTJ) for an energy over several index spaces";
            return nullptr;
        }
        for (int sp : m.unknown_spaces()) nflags += pixels(m.spaces[sp]);
        if (nflags > (1LL << 31) / 16) { *err = "generic: index spaces too large"; return nullptr; }
    }
    // compile (and cache) the kernels here so that a compile error is a NULL plan, as the
    // reference returns nil on errors in the energy (o.t:1526), not a fail-stop
    {
        gen::GModel mc;
        std::string e2;
        gen::build_model(spec.text, &mc, &e2);
        const std::string code = gen::generate(mc, opts.double_precision, gather_offsets_fit_32(mc, s, opts.double_precision)).code;
        std::lock_guard<std::mutex> lk(g_mu);
        if (!code_cache().count(code)) {
            std::string obj, log;
            if (!rtc_compile(code, &obj, &log)) {
                *err = "generic: generated kernels failed to compile:\n" + log;
                return nullptr;
            }
            code_cache()[code] = obj;
        }
    }
    Domain dom{(int)npix, 1, 0, 1, 0, 1};
    if (m.multi()) dom = Domain{(int)nflags, 1, 0, 1, 0, 1};
    else if (ud.size() == 2) {   // image rows: StencilPlan may split them into slabs
        const int W = (int)s.dim_values[m.dims[ud[0]].index], H = (int)s.dim_values[m.dims[ud[1]].index];
        dom = Domain{W, H, 0, H, 0, H};
    }
    if (opts.double_precision) return make_stencil_plan<GenericOp<double>>(s, opts, dom, err);
    return make_stencil_plan<GenericOp<float>>(s, opts, dom, err);
}

// Generated source for `text` (tests / inspection): length, or -1 + message in buf.
int generic_source(const std::string& text, bool dbl, std::string* out, bool off32) {
    gen::GModel m;
    std::string err;
    if (!gen::build_model(text, &m, &err)) { *out = err; return -1; }
    if (!m.unsupported.empty()) { *out = "unsupported: " + m.unsupported; return -1; }
    *out = gen::generate(m, dbl, off32).code;
    return (int)out->size();
}

// What generate() emitted beside the gathers (tests / inspection; tools/gen_dump.cpp prints
// the same fields).
int generic_forms(const std::string& text, bool dbl, std::string* out) {
    gen::GModel m;
    std::string err;
    if (!gen::build_model(text, &m, &err)) { *out = err; return -1; }
    if (!m.unsupported.empty()) { *out = "unsupported: " + m.unsupported; return -1; }
    const gen::GenSource gs = gen::generate(m, dbl);
    char line[256];
    snprintf(line, sizeof line,
             "has_tiled=%d tiles_x=%d tiles_y=%d has_strip=%d strip_cols=%d has_jtf_strip=%d jtf_strip_cols=%d "
             "has_cost_strip=%d cost_strip_cols=%d",
             (int)gs.has_tiled, gs.tiles_x, gs.tiles_y, (int)gs.has_strip, gs.strip_cols, (int)gs.has_jtf_strip,
             gs.jtf_strip_cols, (int)gs.has_cost_strip, gs.cost_strip_cols);
    *out = line;
    return (int)out->size();
}

// One line per residual template: "<domain> <support size> <expression>" (tests).
int generic_describe(const std::string& text, std::string* out) {
    gen::GModel m;
    std::string err;
    if (!gen::build_model(text, &m, &err)) { *out = err; return -1; }
    std::string s;
    auto space = [&](int sp) {   // "{W,H}"
        std::string o = "{";
        for (size_t k = 0; k < m.spaces[sp].size(); ++k) o += (k ? "," : "") + m.dims[m.spaces[sp][k]].name;
        return o + "}";
    };
    for (auto& r : m.residuals) {
        // several index spaces: a centred template names its space, a graph template its slots'
        std::string dom = r.graph < 0 ? std::string("centred") : "graph" + std::to_string(r.graph);
        if (m.multi() && r.graph < 0) dom += space(r.space);
        if (m.multi() && r.graph >= 0) {
            const gen::GGraph& g = m.graphs[r.graph];
            dom += "{";
            for (size_t k = 0; k < g.slot_names.size(); ++k) dom += (k ? "," : "") + g.slot_names[k] + ":" + space(g.slot_space[k]);
            dom += "}";
        }
        s += dom + " " + std::to_string(r.unknowns.size()) + " " + m.pool.str(r.expr) + "\n";
    }
    // RobustEnergy statements: "loss<g> graph<id> <kind> scale=<a | param name> residuals=<R>"
    for (size_t g = 0; g < m.loss.size(); ++g) {
        const gen::GLossGroup& L = m.loss[g];
        char a[64];
        snprintf(a, sizeof a, "%g", L.scale);
        s += "loss" + std::to_string(g) + " graph" + std::to_string(L.graph) + " " +
             (L.kind == gen::GLossGroup::Huber ? "huber" : "cauchy") + " scale=" +
             (L.scale_param >= 0 ? "param " + m.params[L.scale_param].name : std::string(a)) + " residuals=" +
             std::to_string(L.residuals.size()) + "\n";
    }
    *out = s;
    return (int)m.residuals.size();
}

int generic_plan_check(const std::string& text, std::string* why) {
    gen::GModel m;
    if (!gen::build_model(text, &m, why)) return -1;
    std::string r = gen::explicit_refusal(m);
    if (r.empty()) r = gen::normal_refusal(m);
    if (r.empty()) return 0;
    *why = "generic: " + r;
    return 1;
}

// Compile check without a device (hiprtc only): 0 ok, else -1 + log.
int generic_compile_check(const std::string& text, bool dbl, std::string* log) {
    std::string code;
    if (generic_source(text, dbl, &code) < 0) { *log = code; return -1; }
    std::string obj;
    if (!rtc_compile(code, &obj, log)) return -1;
    // graph energies: also the 32-bit gather form plans take below 2 GiB
    if (code.find("a.gnb[") == std::string::npos) return 0;
    if (generic_source(text, dbl, &code, true) < 0) { *log = code; return -1; }
    return rtc_compile(code, &obj, log) ? 0 : -1;
}

}  // namespace optamd
