// stencil_plan.h — host side of the generic image-domain GN / LM solver
// (stencil_driver.h kernels + a family operator). Control flow follows the
// reference's init / step exactly (API/src/solverGPUGaussNewton.t:1766-2349),
// including the LM trust-region update and its early exits.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>
#include "csr.h"
#include "dense_cholesky.h"
#include "stencil_driver.h"

namespace optamd {

// Device pointers of the unknown images (VecLayout order).
template <typename T>
struct UnknownPtrs {
    T* x[4];
};

// X += delta on the active pixels (PCGLinearUpdate, :854-859); LM also keeps the
// previous unknowns (savePreviousUnknowns :882-887) for revertUpdate (:864-869).
template <typename T, bool SAVE>
__global__ __launch_bounds__(kBlock) void update_images_kernel(VecLayout L, const uint8_t* __restrict__ flags,
                                                               UnknownPtrs<T> X, const T* __restrict__ delta,
                                                               T* __restrict__ prev, long long pix_lo,
                                                               long long pix_hi) {
    const long long n = L.off[L.nimg];
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e0 = (long long)blockIdx.x * blockDim.x + threadIdx.x; e0 < n; e0 += kIlp * stride) {
        bool on[kIlp];
        T* xp[kIlp];
        T xv[kIlp], dv[kIlp];
#pragma unroll
        for (int u = 0; u < kIlp; ++u) {   // kIlp elements' loads in flight together
            const long long e = e0 + u * stride;
            const bool in = e < n;
            int k = 0;
            long long local = 0;
            const long long px = in ? L.locate(e, &k, &local) : 0;
            on[u] = in && px >= pix_lo && px < pix_hi && (flags[px] & 1);
            xp[u] = X.x[k] + local;
            xv[u] = *xp[u];
            dv[u] = delta[in ? e : 0];
        }
#pragma unroll
        for (int u = 0; u < kIlp; ++u) {
            if (!on[u]) continue;
            if (SAVE) prev[e0 + u * stride] = xv[u];
            *xp[u] = xv[u] + dv[u];
        }
    }
}
template <typename T>
__global__ __launch_bounds__(kBlock) void revert_images_kernel(VecLayout L, const uint8_t* __restrict__ flags,
                                                               UnknownPtrs<T> X, const T* __restrict__ prev,
                                                               long long pix_lo, long long pix_hi) {
    const long long n = L.off[L.nimg];
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n;
         e += (long long)gridDim.x * blockDim.x) {
        int k;
        long long local;
        const long long px = L.locate(e, &k, &local);
        if (px < pix_lo || px >= pix_hi || !(flags[px] & 1)) continue;
        X.x[k][local] = prev[e];
    }
}

// Op contract (see poisson.hip):
//   using T; static constexpr const char* kName, kApplyName;
//   static constexpr bool kSlabs                          — row-slab decomposition allowed
//   Op(const ProblemSpec&, const StateOptions&, Domain)   — roles from declarations
//   VecLayout layout() const; int halo() const;
//   void bind(void** params, hipStream_t)                 — pointers + scalar params
//   T* unknown(int k)                                     — device unknown image k
//   void precompute(hipStream_t)                           — materialise ComputedArrays
//                     (init, after each update and after a revert: :1876, 2242, 2284)
//   void computed_planes(std::vector<HaloPlane>&)          — what precompute writes
//   void jtf(T* r, T* diag, uint8_t* flags, hipStream_t)  — r = -J^T F, diag(J^T J), flags
//   void apply(const T* p, T* Ap, const T* dadd, const int* stop, ReduceSlot, hipStream_t)
//                     — Ap = J^T J p (+ dadd p), sum p.Ap; returns early if *stop
//   void cost(ReduceSlot, hipStream_t); void model_cost(const T* delta, ReduceSlot, hipStream_t)
//   void unbind(hipStream_t)                               — copy unknowns back (host mode)
// All stencil kernels cover the owned rows [y_lo, y_hi) of the Domain and read up to
// halo() rows beyond them.
//
// Optional methods, each with the trait that finds it and the methods that come with it
// (described at the traits below):
//   HasDumpJ               dump_j(rowPtr, colInd, val, s); jacobian_rows(), jacobian_nnz()
//   HasApplySplit          can_split(); apply_split(part, ...apply's arguments)
//   HasApplySums           apply_sums(part, p, Ap, dadd, stop, rs, r, w, s, e0, e1)
//   HasFusedStep3          step3_fused(pre, r, p, sc, i_num, i_den, use_pre, stop, s);
//                          apply_prepared(...apply's arguments)
//   HasApplyExt            apply_ext(...apply's arguments, e0, e1)
//   HasSlabRefusal         slab_refusal()
//   HasRefreshCaches       refresh_caches(s)
//   HasTopologyGeneration  topology_generation()
//   HasCaptureKey          capture_key(key)
//   HasBlockPre            block_pre(); block_entries(), set_block_buffer, block_layout,
//                          block_init, block_step2, block_half2, block_apply
//   HasSchur               schur(); schur_entries(), set_schur_buffers, eliminated, schur_rhs,
//                          schur_elim, schur_apply, schur_back
//   HasExplicitMatrix      matrix_form(); matrix_symbolic_stale, matrix_symbolic, matrix_eblk,
//                          matrix_assemble, matrix_spmv, matrix_shape, matrix_copy, matrix_key,
//                          symbolic_info
// A trait looks for its first method by NAME only (none of these is overloaded or a
// template): an Op whose signature drifts fails to compile where the driver calls it,
// instead of losing the feature without a word. Each Op's source asserts the traits it
// claims.
//
// Row-slab decomposition: each rank owns rows [y_lo, y_hi) and holds
// halo() rows of each neighbour. The flat PCG kernels run over the whole memory slab:
// the init kernels zero pre / p / r / b / CtC outside the owned rows (and the stencil
// kernels write Ap only there), so every flat reduction sums owned elements only. The
// exchanges are: unknowns after bind / update / revert, computed arrays after each
// precompute, flags after J^T F, p before each apply (delta before an apply of delta
// and before the model cost); every scalar is all-reduced right after its kernel.
#define OPTAMD_OP_TRAIT(Trait, method)                                                          \
    template <class Op, class = void>                                                           \
    struct Trait : std::false_type {};                                                          \
    template <class Op>                                                                         \
    struct Trait<Op, std::void_t<decltype(&Op::method)>> : std::true_type {}

// The materialized path (useMaterializedJTJ, csr.h): long long jacobian_rows() const,
// jacobian_nnz() const; void dump_j(int* rowPtr, int* colInd, T* val, hipStream_t) — J in
// CSR (saveJToCRS).
OPTAMD_OP_TRAIT(HasDumpJ, dump_j);

// Ops whose apply can run as interior + boundary launches (row slabs: the halo refresh
// of p overlaps the interior part): bool can_split() const; void apply_split(int part,
// ... apply's arguments) with part 1 = no halo reads, 2 = the rest, 0 = everything.
OPTAMD_OP_TRAIT(HasApplySplit, can_split);

// Ops whose apply can also reduce the fused PCG step's sums (shape_from_shading):
// apply_sums(part, p, Ap, dadd, stop, rs, r, w, stream, e0, e1) reduces {p.Ap, r.W Ap,
// Ap.W Ap, r.W r} (fp64) into rs; the driver then runs PCGStep2 + PCGStep3 as ONE pass
// (step23_kernel, beta's numerator from the identity over those sums) and, on row slabs,
// one all-reduce per PCG iteration.
OPTAMD_OP_TRAIT(HasApplySums, apply_sums);

// Ops that fold PCGStep3 into the first pass of their next apply (ARAP: p = z + beta p
// per vertex, then K of the new p): step3_fused(pre, r, p, sc, i_num, i_den, use_pre,
// stop, s) replaces step3_kernel; apply_prepared(...apply's arguments) is the apply
// without that first pass.
OPTAMD_OP_TRAIT(HasFusedStep3, step3_fused);

// Optional Op::apply_ext(p, Ap, dadd, stop, rs, stream, e0, e1): the apply with HIP
// events attached to its launch (hipExtLaunchKernelGGL), so the per-kernel timer measures
// the kernel itself instead of event records around the launch.
OPTAMD_OP_TRAIT(HasApplyExt, apply_ext);

// Ops that decide per energy whether row slabs are possible: std::string slab_refusal()
// const, the reason or "".
OPTAMD_OP_TRAIT(HasSlabRefusal, slab_refusal);

// Ops that keep private per-step caches of values derived from the bound arrays
// (GenericOp: transcendentals of centred and graph-slot reads, and the sample caches —
// sampled images and their gradient images at the unknowns' coordinates): refresh_caches
// (stream) recomputes them at the start of every Step from the arrays as bound at THIS
// Step. The reference evaluates those values inline from the arrays at every Step
// (setGPUptr, solverGPUGaussNewton.t:2001), so a caller may rewrite or rebind arrays —
// the unknowns included — between Steps (Opt.h:64-65). Caches that depend on the unknowns
// are rebuilt after each update and revert as well (they ride with precompute). The
// energy's ComputedArrays themselves keep the reference's schedule (init, after update,
// after revert) and are NOT refreshed at Step start.
OPTAMD_OP_TRAIT(HasRefreshCaches, refresh_caches);

// Ops whose Jacobian's column structure comes from bound vertex arrays (ArapOp, GenericOp
// with graphs): topology_generation() is a counter the Op bumps whenever bind finds the
// arrays' content fingerprint changed and rebuilds its incidence lists (graph_util.h). The
// materialized path keeps everything it derives from J's sparsity (J^T pattern, J^T J
// pattern, SELL copies, product map) for as long as that counter stands, and derives it
// again at the first Step or apply after it moved (materialize below): the Step-boundary
// contract lets a caller rewrite or rebind the vertex arrays between Steps. Image families
// have no such method and build their patterns once per plan.
OPTAMD_OP_TRAIT(HasTopologyGeneration, topology_generation);

// Ops that describe their own hipGraph capture gate and key (GenericOp: the kernel
// argument block the generated launches receive) instead of the declaration parser's.
OPTAMD_OP_TRAIT(HasCaptureKey, capture_key);

// Ops with a block preconditioner (GenericOp for UsePreconditioner("block")): block_pre()
// says whether this energy asked for it; then jtf also fills the plan's block buffer
// (set_block_buffer, block_entries() values) and block_init / block_step2 / block_half2 /
// block_apply are the per-element PCG kernels that replace the scalar z = pre r: z goes to
// its own vector, and PCGStep3 runs on it with use_pre = 0.
OPTAMD_OP_TRAIT(HasBlockPre, block_pre);

// Ops that can eliminate one group of unknowns (GenericOp for Eliminate(X, ...)): schur()
// says whether this energy asked for it (then block_pre() holds too). PCG then runs on the
// Schur complement S = B - E M^-1 E^T over the retained unknowns, in the full vector layout
// with the eliminated entries of p, r, z, Ap and delta exactly zero: pcg_loop's block stages
// as they are, with the apply replaced by schur_elim (w = -M^-1 E^T p) + schur_apply (B p +
// E w); before the loop schur_rhs (M_e^-1, the stash of b_e, w = M^-1 b_e) and one schur_apply
// of p = 0 give the reduced right-hand side b_r - E M^-1 b_e; after it schur_back writes
// delta_e = M^-1 (b_e - E^T delta_r), and the update, model cost and cost see the full delta.
OPTAMD_OP_TRAIT(HasSchur, schur);

// Ops that can assemble the matrix PCG runs on in block-CSR (GenericOp): matrix_form() says
// which one this energy asked for — S of ReducedSystem("explicit") (then schur() holds) or
// H = J^T J of NormalMatrix("explicit") (then block_pre() holds and schur() does not). Once per
// Step, before block_init inverts the blocks the assembly reads — S after schur_rhs has left
// M_e^-1 in the block buffer, H after jtf has left the diagonal blocks there — matrix_symbolic
// (only after a re-wiring), matrix_eblk and matrix_assemble build it; every apply of the PCG
// loop — and the residual reset's, and apply_reduced's / apply_jtj's — is then matrix_spmv, with
// schur_apply's / apply's contract. LM's diagonal is not part of the matrix: the SpMV adds dadd p.
// The timer entries keep the form's name: schur_* / normal_* + symbolic, eblk, assemble, spmv.
enum class MatrixForm { None, Schur, Normal };
OPTAMD_OP_TRAIT(HasExplicitMatrix, matrix_form);

// Ops that choose among several forms of their kernels (GenericOp: gather, LDS tiles, register
// strips): std::string generated_forms() const, the forms this plan launches.
OPTAMD_OP_TRAIT(HasGeneratedForms, generated_forms);

// Ops with robust losses (GenericOp for RobustEnergy): has_loss() says whether this energy has
// the statement. loss_weights(s) caches one weight sqrt(rho'(s)) per edge and loss group at the
// bound unknowns; every kernel of the linear system reads it. It follows precompute (Init, after
// update, after revert, the stand-alone entry points) and the per-Step refresh, after both:
// arrays, Params and unknowns may change between Steps. Cost and model cost evaluate rho
// themselves. loss_groups / eval_loss_rho1: OptAMD_PlanLossGroups / OptAMD_EvalLossWeights.
OPTAMD_OP_TRAIT(HasLossWeights, loss_weights);
#undef OPTAMD_OP_TRAIT

// r -= Ap (and b = r, LM): the reduced right-hand side from Ap = E M^-1 b_e
template <typename T>
__global__ __launch_bounds__(kBlock) void schur_sub_kernel(long long n, T* __restrict__ r, const T* __restrict__ Ap,
                                                           T* __restrict__ b) {
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const T v = r[e] - Ap[e];
        r[e] = v;
        if (b) b[e] = v;
    }
}

// z = pre r (OptAMD_ApplyPreconditioner on a scalar plan)
template <typename T>
__global__ __launch_bounds__(kBlock) void scale_kernel(long long n, const T* __restrict__ pre, const T* __restrict__ r,
                                                       T* __restrict__ z) {
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x)
        z[e] = pre[e] * r[e];
}
// x = v
template <typename T>
__global__ __launch_bounds__(kBlock) void fill_kernel(long long n, T v, T* __restrict__ x) {
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x)
        x[e] = v;
}

template <class Op>
class StencilPlan final : public Plan {
public:
    using T = typename Op::T;
    StencilPlan(const ProblemSpec& spec, const StateOptions& opts, Domain dom) : Plan(spec, opts), dom_(dom) {
        lm_ = spec.lm();
        stop_ = (int*)dmalloc(64);
        OPT_HIP_CHECK(hipMemset(stop_, 0, 64));
        timer_.apply_name = Op::kApplyName;
        allocate();
    }
    ~StencilPlan() override {
        OPT_HIP_CHECK(hipStreamSynchronize(stream_));
        release();
        dfree(stop_);
    }

    long long unknown_count() const override { return n_; }
    std::string family() const override { return Op::kName; }
    std::string apply_kernel_name() const override { return mat_ ? mat_->apply_name() : Op::kApplyName; }
    int generated_forms(std::string* out) const override {
        if constexpr (HasGeneratedForms<Op>::value) {
            // (a materialized plan's applies are SpMVs of the dumped J, not the apply form named here)
            *out = op_->generated_forms() + (mat_ ? " materialized=1" : " materialized=0");
            return 0;
        }
        return -1;
    }
    int halo() const override { return op_->halo(); }
    int unknown_layout(int max_images, long long* offset, long long* elements, int* channels) const override {
        for (int k = 0; k < L_.nimg && k < max_images; ++k) {
            if (offset) offset[k] = L_.off[k];
            if (elements) elements[k] = (L_.off[k + 1] - L_.off[k]) / L_.ch[k];
            if (channels) channels[k] = L_.ch[k];
        }
        return L_.nimg;
    }

    std::string set_decomposition(Comm* comm, int y_lo, int y_hi) override {
        if (!Op::kSlabs) return std::string(Op::kName) + ": no row-slab decomposition (data-dependent reads)";
        if constexpr (HasSlabRefusal<Op>::value) {
            const std::string why = op_->slab_refusal();
            if (!why.empty()) return why;
        }
        if (opts_.host_buffers) return "row-slab decomposition needs backend_cuda (device arrays)";
        if (opts_.materialized) return "row-slab decomposition of the materialized Jacobian path is not supported";
        const int h = op_->halo();
        if (y_lo < 0 || y_hi > dom_.H || y_hi - y_lo < h) return "invalid slab rows";
        comm_ = comm;
        OPT_HIP_CHECK(hipStreamSynchronize(stream_));
        release();
        dom_.y_lo = y_lo;
        dom_.y_hi = y_hi;
        dom_.y_mem0 = std::max(0, y_lo - h);
        dom_.mem_rows = std::min(dom_.H, y_hi + h) - dom_.y_mem0;
        allocate();
        initialised_ = false;
        return "";
    }

    void init(void** params) override {
        begin_call();
        op_->bind(params, stream_);
        exchange_unknowns();
        // reference init: LM parameters copied into the plan (:1863-1872), precompute,
        // prevCost = cost; PCGInit1 is redone by every step
        radius_ = sp_.trust_region_radius;
        decrease_ = sp_.radius_decrease_factor;
        precompute();
        tbegin("cost"); op_->cost(red_.slot(nb(), kScCost), stream_); tend();
        allreduce(kScCost, 1);
        prev_cost_ = read(kScCost);
        n_iter_ = 0;
        initialised_ = true;
        end_call();
    }

    int step(void** params) override {
        if (!initialised_) init(params);
        if (n_iter_ >= sp_.nIterations) {
            cleanup_log();
            return 0;
        }
        begin_call();
        op_->bind(params, stream_);
        exchange_unknowns();
        if constexpr (HasRefreshCaches<Op>::value) {
            if (op_->refresh_caches(stream_)) exchange_computed();
        }
        loss_weights();
        const int Lit = std::max(0, sp_.lIterations);
        red_.ensure(std::max(op_->stencil_blocks(), 4096), 4, kScBase + kSlots * (Lit + 2));
        OPT_HIP_CHECK(hipMemsetAsync(stop_, 0, 64, stream_));
        OPT_HIP_CHECK(hipMemsetAsync(delta_, 0, sizeof(T) * n_, stream_));   // PCGInit1: delta = 0
        linear_init(rz(0), true);   // PCGInit1 (+ LM diagonal)
        if (lm_) OPT_HIP_CHECK(hipMemsetAsync(red_.scalars + kScQ0, 0, sizeof(double), stream_));
        schur_prepare(true);   // (delta_ = 0 here: the p of the reduced right-hand side's apply)
        if (matrix_ == MatrixForm::Normal) explicit_prepare();   // H from jtf's diagonal blocks (S: in schur_prepare)
        if constexpr (HasBlockPre<Op>::value)
            if (block_) {   // M_e^-1 in place of the blocks, z_0 = M^-1 r, p_0 = z_0, rz_0
                tbegin("blk_init");
                op_->block_init(r_, pre_, CtC_, z_, p_, lm_ ? 1 : 0, red_.slot(nb(), rz(0)), stream_);
                tend();
            }
        allreduce(rz(0), 1);
        const int* stop = lm_ ? stop_ : nullptr;
        if (mat_) materialize();   // cusparseOuter (:2068): J, J^T (, J^T J) at the current X
        if (!direct_step(Lit) && pcg_graph_begin(params, Lit)) {
            pcg_loop(Lit, stop);
            pcg_graph_end();
        }
        if constexpr (HasSchur<Op>::value)
            if (schur_ && Lit > 0) {   // delta_e = M^-1 (b_e - E^T delta_r); never skipped by LM's stop flag
                tbegin("schur_back");
                op_->schur_back(delta_, stream_);
                tend();
            }
        if (!lm_) {
            if (Lit > 0) update(false);
            precompute();
            tbegin("cost"); op_->cost(red_.slot(nb(), kScCost), stream_); tend();
            allreduce(kScCost, 1);
            const double c = read(kScCost);
            op_->unbind(stream_);
            end_call();
            prev_cost_ = c;
            ++n_iter_;
            return 1;
        }
        return lm_finish_step();
    }

    // PCG inner loop (PCGStep1-3, :607-845) of one step; launches only, no host sync. One
    // iteration is the stages below (the private pcg_* members, each picks its variant), with
    // a row-slab run's all-reduces between them.
    void pcg_loop(int Lit, const int* stop) {
        if constexpr (HasApplySums<Op>::value)
            if (!mat_ && (fuse23_ == 1 || (fuse23_ == 2 && distributed()))) {
                pcg_loop_fused(Lit, stop);
                return;
            }
        for (int i = 0; i < Lit; ++i) {
            // the zeta test rides in the kernel that reduces q (one GPU), else its own launch
            const ZetaArgs z = zeta_args(i);
            pcg_apply(i, stop);
            allreduce(pap(i), 1);
            if (reset_iteration(i)) {   // the classic halves, the reference's unguarded division (:742)
                pcg_half1<false>(i, stop);
                pcg_reset_apply(stop);
                pcg_half2(i, stop, z);
            } else {
                pcg_step2(i, stop, z);
            }
            allreduce(rz(i + 1), lm_ ? 2 : 1);   // rz and q sit side by side
            if (!pcg_step3_fused(i, stop)) pcg_step3<false>(i, stop);
            if (lm_ && !z.on) pcg_zeta(i);
            OPT_HIP_CHECK(hipGetLastError());
        }
    }

    // The PCG loop with PCGStep2 + PCGStep3 as one pass (HasApplySums, UsePreconditioner):
    // per iteration the apply (+ its four sums) and step23_kernel; on row slabs ONE
    // all-reduce per iteration — step23's rz / q ride in the next apply's call — and LM's
    // zeta test on the all-reduced q before the next step23 (the apply in between is
    // wasted when it stops: the reference would have left the loop before it). Residual-reset
    // iterations (LM) run the classic sequence.
    void pcg_loop_fused(int Lit, const int* stop) {
        bool pending = false;   // rz(i) / q(i) of the previous step23 not all-reduced yet
        for (int i = 0; i < Lit; ++i) {
            const ZetaArgs z = zeta_args(i);
            pcg_apply_sums(i, stop);
            if (distributed()) {
                allreduce(pending ? rz(i) : pap(i), pending ? 6 : 4);
                if (pending && lm_) pcg_zeta(i - 1);   // the previous iteration's exit test on the global q
                pending = false;
            }
            if (reset_iteration(i)) {   // the classic halves with step23's guards (a zero step / beta = 0)
                pcg_half1<true>(i, stop);
                pcg_reset_apply(stop);
                pcg_half2(i, stop, z);
                allreduce(rz(i + 1), 2);
                pcg_step3<true>(i, stop);
                if (!z.on) pcg_zeta(i);
                OPT_HIP_CHECK(hipGetLastError());
                continue;
            }
            pcg_step23(i, stop, z);
            if (distributed()) pending = true;
        }
    }

    // The PCG loop of a launch-bound (small) problem costs more in launches than in
    // kernel time (poisson 512^2: ~30 launches of a few us each per step), so on one GPU
    // it is captured once as a hipGraph and replayed. The graph is keyed on everything
    // its launches bake in: the bound arrays and scalar parameter values, the plan's
    // buffers and lIterations; for generated kernels, the whole argument block they
    // receive (Op::capture_key, built from the lowered model, not the declaration
    // parser). Not used with timers (per-kernel events), row slabs (RCCL calls between
    // launches), the materialized path, or graph-domain energies (their adjacency may be
    // rebuilt on bind). OPT_AMD_NO_GRAPH=1 turns it off.
    // Returns true when the caller must issue the launches (eagerly or under capture).
    bool pcg_graph_begin(void** params, int Lit) {
        bool graphs = !spec_.graphs.empty();
        std::vector<unsigned long long> op_key;
        if constexpr (HasCaptureKey<Op>::value) graphs = !op_->capture_key(&op_key);
        if (distributed() || mat_ || timer_.mode || graphs || Lit <= 0 || graph_off_) {
            drop_graph();
            return true;
        }
        std::vector<unsigned long long> key{(unsigned long long)Lit, (unsigned long long)(uintptr_t)red_.scalars,
                                            (unsigned long long)(uintptr_t)red_.partials,
                                            (unsigned long long)(uintptr_t)red_.ticket,
                                            (unsigned long long)(uintptr_t)op_.get(),
                                            (unsigned long long)(uintptr_t)p_};
        key.insert(key.end(), op_key.begin(), op_key.end());
        if (block_) {   // the block path's launches also bake in its two buffers
            key.push_back((unsigned long long)(uintptr_t)blk_);
            key.push_back((unsigned long long)(uintptr_t)z_);
        }
        if (schur_) key.push_back((unsigned long long)(uintptr_t)w_);
        if constexpr (HasExplicitMatrix<Op>::value)
            if (matrix_ != MatrixForm::None) op_->matrix_key(&key);
        if constexpr (!HasCaptureKey<Op>::value) {
            for (const DeclImage& im : spec_.images)   // arrays by address, scalars by value (below)
                if (im.index >= 0 && im.index < spec_.n_params_total)
                    key.push_back((unsigned long long)(uintptr_t)params[im.index]);
            for (const DeclParam& d : spec_.params) {
                unsigned long long v = 0;
                if (d.index >= 0 && d.index < spec_.n_params_total && params[d.index])
                    memcpy(&v, params[d.index], d.type == "double" ? 8 : 4);
                key.push_back(v);
            }
        }
        {   // solver parameters the loop bakes in (Opt_SetSolverParameter may change them)
            unsigned long long qt = 0;
            memcpy(&qt, &sp_.q_tolerance, sizeof(sp_.q_tolerance) <= 8 ? sizeof(sp_.q_tolerance) : 8);
            key.push_back(qt);
            key.push_back((unsigned long long)sp_.residual_reset_period);
        }
        if (graph_exec_ && key == graph_key_) {
            OPT_HIP_CHECK(hipGraphLaunch(graph_exec_, stream_));
            return false;
        }
        drop_graph();
        graph_key_ = key;
        OPT_HIP_CHECK(hipStreamBeginCapture(stream_, hipStreamCaptureModeRelaxed));
        capturing_ = true;
        return true;
    }
    void pcg_graph_end() {
        if (!capturing_) return;
        capturing_ = false;
        hipGraph_t g = nullptr;
        OPT_HIP_CHECK(hipStreamEndCapture(stream_, &g));
        OPT_HIP_CHECK(hipGraphInstantiate(&graph_exec_, g, nullptr, nullptr, 0));
        OPT_HIP_CHECK(hipGraphDestroy(g));
        OPT_HIP_CHECK(hipGraphLaunch(graph_exec_, stream_));
    }
    void drop_graph() {
        if (graph_exec_) OPT_HIP_CHECK(hipGraphExecDestroy(graph_exec_));
        graph_exec_ = nullptr;
        graph_key_.clear();
    }

    // ---- LM: model cost, speculative update, accept / reject (:2229-2292)
    int lm_finish_step() {
        const int Lit = std::max(0, sp_.lIterations);
        exchange_vec(delta_);
        tbegin("model_cost"); op_->model_cost(delta_, red_.slot(nb(), kScModel), stream_); tend();
        if (Lit > 0) update(true);
        precompute();
        tbegin("cost"); op_->cost(red_.slot(nb(), kScCost), stream_); tend();
        allreduce(kScModel, 2);   // model cost and cost
        double h[2];
        OPT_HIP_CHECK(hipMemcpyAsync(h, red_.scalars + kScModel, sizeof(h), hipMemcpyDeviceToHost, stream_));
        OPT_HIP_CHECK(hipStreamSynchronize(stream_));
        const T model_cost = (T)h[0], new_cost = (T)h[1];
        const T prev = (T)prev_cost_;
        const T model_change = prev - model_cost;
        log_solver(" cost=%f \n", (double)prev);   // computeModelCostChange (:1505-1513)
        log_solver(" model_cost=%f \n", (double)model_cost);
        log_solver(" model_cost_change=%f \n", (double)model_change);
        const T cost_change = prev - new_cost;
        const T rel = cost_change / model_change;
        int ret = 1;
        if (cost_change >= (T)0 && rel > (T)sp_.min_relative_decrease) {
            const T abs_tol = prev * (T)sp_.function_tolerance;
            if (cost_change <= abs_tol) {
                ret = 0;   // function tolerance reached (prevCost is left as it was, :2254-2258)
                log_solver("\nFunction tolerance reached, exiting\n");
            } else {
                const T qv = rel;
                const T min_factor = (T)(1.0 / 3.0);
                const T tmp = (T)1 - (T)std::pow((double)((T)2 * qv - (T)1), 3.0);
                float rad = (float)((T)radius_ / std::max(min_factor, tmp));
                radius_ = std::min(rad, sp_.max_trust_region_radius);
                decrease_ = 2.0f;
                prev_cost_ = (double)new_cost;
            }
        } else {
            if (Lit > 0) revert();
            precompute();
            radius_ = radius_ / decrease_;
            log_solver(" trust_region_radius=%f \n", (double)radius_);
            decrease_ = 2.0f * decrease_;
            if (radius_ <= sp_.min_trust_region_radius) {
                ret = 0;
                log_solver("\nTrust_region_radius is less than the min, exiting\n");
            } else {
                log_solver("REVERT\n");
            }
        }
        op_->unbind(stream_);
        end_call();
        if (ret) ++n_iter_;
        else cleanup_log();
        return ret;
    }

    int eval_jtf(void** params, void* r, void* pre, double* rzv) override {
        begin_call();
        prepare(params);
        op_->jtf((T*)r, diag_, flags_, stream_);
        hipLaunchKernelGGL((gn_init_kernel<T>), dim3(fg()), dim3(kBlock), 0, stream_, L_, (const uint8_t*)flags_,
                           (T*)r, (const T*)diag_, (T*)pre, p_, spec_.use_preconditioner ? 1 : 0, pix_lo(),
                           pix_hi(), red_.slot(fg(), kScTmp));
        allreduce(kScTmp, 1);
        *rzv = read(kScTmp);
        end_call();
        return 0;
    }
    // z = M^-1 r at the current unknowns for the caller's r: the GN form on a GN plan, the LM
    // form with the current trust-region radius on an LM plan (the scalar init kernels run as
    // in step(); every buffer they write is rebuilt by the next step).
    int apply_preconditioner(void** params, const void* rin, void* zout) override {
        begin_call();
        prepare(params);
        red_.ensure(std::max(op_->stencil_blocks(), 4096), 4, kScBase + kSlots * (std::max(0, sp_.lIterations) + 2));
        linear_init(kScTmp, false);
        schur_prepare(false);   // (a Schur plan's eliminated blocks: inverted by their own rule)
        bool blk = false;
        if constexpr (HasBlockPre<Op>::value)
            if (block_) {
                op_->block_init(r_, pre_, CtC_, z_, p_, lm_ ? 1 : 0, red_.slot(nb(), kScTmp), stream_);
                op_->block_apply((const T*)rin, (T*)zout, stream_);
                blk = true;
            }
        if (!blk)
            hipLaunchKernelGGL((scale_kernel<T>), dim3(fg()), dim3(kBlock), 0, stream_, n_, (const T*)pre_,
                               (const T*)rin, (T*)zout);
        OPT_HIP_CHECK(hipGetLastError());
        end_call();
        return 0;
    }
    int eliminated(int max_images, int* flag) const override {
        for (int k = 0; k < L_.nimg && k < max_images; ++k)
            if (flag) flag[k] = 0;
        if constexpr (HasSchur<Op>::value)
            if (schur_) return op_->eliminated(max_images, flag);
        return L_.nimg;
    }
    // Sp = (B - E M^-1 E^T) p at the current unknowns (LM: with CtC_r p and M = C + CtC_e at the
    // current radius), 0 in the eliminated entries, whatever the caller's p holds there: the
    // same preparation as apply_preconditioner, then one reduced apply.
    int apply_reduced(void** params, const void* pin, void* Sp) override {
        if constexpr (HasSchur<Op>::value) {
            if (!schur_) return 1;
            begin_call();
            reduced_prepare(params);
            op_->block_init(r_, pre_, CtC_, z_, p_, lm_ ? 1 : 0, red_.slot(nb(), kScTmp), stream_);
            schur_apply((const T*)pin, (T*)Sp, lm_ ? CtC_ : nullptr, nullptr, red_.slot(nb(), kScTmp));
            end_call();
            return 0;
        }
        return Plan::apply_reduced(params, pin, Sp);
    }
    bool reduced_matrix_shape(long long* rows, int* dim, long long* nnzb) const override {
        return explicit_shape(MatrixForm::Schur, rows, dim, nnzb);
    }
    // S at the current unknowns: the preparation of apply_reduced (whose schur_prepare runs
    // the numeric phase), then the block-CSR copied out; every buffer the preparation writes
    // is rebuilt by the next step
    int reduced_matrix(void** params, int* rowPtr, int* colInd, void* val) override {
        return explicit_matrix(MatrixForm::Schur, params, rowPtr, colInd, val);
    }
    // what LinearSolver("cholesky") did on this plan so far; -1 on a plan without the statement
    int direct_info(std::string* line) const override {
        if constexpr (HasExplicitMatrix<Op>::value)
            if (matrix_ != MatrixForm::None && op_->direct_solver()) {
                char ratio[40];
                snprintf(ratio, sizeof(ratio), "%.9g", direct_ratio_);
                *line = "n=" + std::to_string(direct_n_) + " tiles=" + std::to_string(direct_n_ ? dense_tile_count(direct_n_) : 0) +
                        " bytes=" + std::to_string(direct_n_ ? dense_bytes(direct_n_, sizeof(T)) : 0) +
                        " factorisations=" + std::to_string(direct_factorisations_) + " fallbacks=" +
                        std::to_string(direct_fallbacks_) + " reason=" + direct_reason_ + " min_pivot_ratio=" + ratio +
                        " covariances=" + std::to_string(covariances_) + " cov_bytes=" + std::to_string(cov_bytes_);
                return 0;
            }
        return Plan::direct_info(line);
    }
    // Blocks of the inverse of S or H at the bound unknowns (OptAMD_Covariance): the assembly of
    // explicit_matrix() — on an LM plan with Eliminate without the diagonal in M_e — then dense_fill
    // without LM's diagonal and with a vector of ones for r, which leaves in the tiles' right-hand
    // side a 1 per active unknown and a 0 per excluded or held one (the gather's mask), the
    // factorisation, and DenseFactor's forward chain, Gram tiles and gather. Shares dense_ with
    // direct_step, which refills it at every Step; writes Ap_ (the ones) and what explicit_matrix()
    // writes, all rebuilt by the next Step; never delta_, the unknowns, the cost or the LM state.
    int covariance(void** params, long long nPairs, const int* rowElem, const int* colElem, void* blocks,
                   std::string* why) override {
        if constexpr (HasExplicitMatrix<Op>::value) {
            if (matrix_ == MatrixForm::None || !op_->direct_solver()) return 1;
            begin_call();
            const int ret = covariance_body(params, nPairs, rowElem, colElem, (T*)blocks, why);
            end_call();
            return ret;
        }
        return Plan::covariance(params, nPairs, rowElem, colElem, blocks, why);
    }
    // what the last symbolic phase of S or H did; -1 on a plan with neither statement
    int symbolic_info(std::string* line) const override {
        if constexpr (HasExplicitMatrix<Op>::value)
            if (matrix_ != MatrixForm::None) return *line = op_->symbolic_info(), 0;
        return Plan::symbolic_info(line);
    }
    bool normal_matrix_shape(long long* rows, int* dim, long long* nnzb) const override {
        return explicit_shape(MatrixForm::Normal, rows, dim, nnzb);
    }
    // H at the current unknowns: bind, J^T F with its diagonal blocks, the numeric phase, then
    // the block-CSR copied out; every buffer this writes is rebuilt by the next step
    int normal_matrix(void** params, int* rowPtr, int* colInd, void* val) override {
        return explicit_matrix(MatrixForm::Normal, params, rowPtr, colInd, val);
    }
    int loss_groups(int max_groups, int* graph, int* residuals, int* kind) const override {
        if constexpr (HasLossWeights<Op>::value) return op_->loss_groups(max_groups, graph, residuals, kind);
        return 0;
    }
    long long loss_group_edges(int group) const override {
        if constexpr (HasLossWeights<Op>::value) return op_->loss_group_edges(group);
        return -1;
    }
    // rho'(s) per edge of one loss group at the bound unknowns; 1 on a plan without the statement
    int eval_loss_weights(void** params, int group, void* weights) override {
        if constexpr (HasLossWeights<Op>::value) {
            if (!op_->has_loss()) return 1;
            begin_call();
            prepare(params);
            op_->eval_loss_rho1(group, (T*)weights, stream_);
            OPT_HIP_CHECK(hipStreamSynchronize(stream_));
            end_call();
            return 0;
        }
        return Plan::eval_loss_weights(params, group, weights);
    }
    int preconditioner_blocks(int max_images, int* group, int* first_row) const override {
        if constexpr (HasBlockPre<Op>::value)
            if (block_) return op_->block_layout(max_images, group, first_row);
        return 0;
    }
    int apply_jtj(void** params, const void* p, void* Ap, double* pAp) override {
        begin_call();
        prepare(params);
        op_->jtf(r_, diag_, flags_, stream_);   // flags for the exclusion mask
        exchange({{(void*)flags_, (size_t)dom_.W}});
        exchange_vec((T*)p);
        if (mat_) {
            materialize();
            mat_apply((const T*)p, (T*)Ap, nullptr, kScTmp);
        } else if (matrix_ == MatrixForm::Normal) {   // the explicit path: H from this call's blocks, then the SpMV
            explicit_prepare();
            explicit_apply((const T*)p, (T*)Ap, nullptr, nullptr, red_.slot(nb(), kScTmp));
        } else {
            tbegin(Op::kApplyName);   // the same timer entry as the PCG loop's applies
            op_->apply((const T*)p, (T*)Ap, nullptr, nullptr, red_.slot(nb(), kScTmp), stream_);
            tend();
        }
        allreduce(kScTmp, 1);
        *pAp = read(kScTmp);
        end_call();
        return 0;
    }
    double eval_cost(void** params) override {
        begin_call();
        prepare(params);
        op_->cost(red_.slot(nb(), kScTmp), stream_);
        allreduce(kScTmp, 1);
        const double c = read(kScTmp);
        end_call();
        return c;
    }
    double time_apply(void** params, const void* p, void* Ap, int reps) override {
        begin_call();
        prepare(params);
        op_->jtf(r_, diag_, flags_, stream_);
        if (mat_) materialize();
        auto run = [&]() {
            if (mat_) mat_apply((const T*)p, (T*)Ap, nullptr, kScTmp);
            else op_->apply((const T*)p, (T*)Ap, nullptr, nullptr, red_.slot(nb(), kScTmp), stream_);
        };
        hipEvent_t e0, e1;
        OPT_HIP_CHECK(hipEventCreate(&e0));
        OPT_HIP_CHECK(hipEventCreate(&e1));
        run();
        OPT_HIP_CHECK(hipEventRecord(e0, stream_));
        for (int i = 0; i < reps; ++i) run();
        OPT_HIP_CHECK(hipEventRecord(e1, stream_));
        OPT_HIP_CHECK(hipEventSynchronize(e1));
        float ms = 0;
        OPT_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        end_call();
        return 1000.0 * ms / std::max(1, reps);
    }

    long long jacobian_shape(long long* rows) const override {
        if constexpr (HasDumpJ<Op>::value) {
            if (rows) *rows = op_->jacobian_rows();
            return op_->jacobian_nnz();
        }
        return Plan::jacobian_shape(rows);
    }
    bool materialized_nonzeros(long long* nnzJ, long long* nnzJTJ) const override {
        if (!mat_) return false;
        if (nnzJ) *nnzJ = mat_->nnz();
        if (nnzJTJ) *nnzJTJ = mat_->nnz_jtj();
        return true;
    }
    int eval_jacobian(void** params, int* rowPtr, int* colInd, void* val) override {
        if constexpr (HasDumpJ<Op>::value) {
            if (distributed() || dom_.mem_rows != dom_.H) return 1;
            begin_call();
            prepare(params);
            op_->jtf(r_, diag_, flags_, stream_);   // families whose J reuses J^T F state (optical_flow)
            op_->dump_j(rowPtr, colInd, (T*)val, stream_);
            end_call();
            return 0;
        }
        return Plan::eval_jacobian(params, rowPtr, colInd, val);
    }

private:
    static constexpr int kScCost = 1, kScModel = 0, kScTmp = 2, kScQ0 = 3, kScBase = 8;
    static constexpr int kScQc = kScQ0 + 1;   // Schur plans: 1/2 b_e.M^-1 b_e, read as q0[1] by the exit test
    // cost sits right after model cost so one 16-byte copy (and one all-reduce) takes both
    // per PCG iteration: rz[i], q[i] (written together by step2 as a pair), pAp[i]
    // iteration i's slots: rz, q, pAp, then (fused PCG step) r.W Ap, Ap.W Ap, r.W r and
    // step23's identity value of rz
    static constexpr int kSlots = 7;
    int rz(int i) const { return kScBase + kSlots * i; }
    int q(int i) const { return kScBase + kSlots * i + 1; }
    int pap(int i) const { return kScBase + kSlots * i + 2; }
    int nb() const { return op_->stencil_blocks(); }
    int fg() const { return flat_grid(n_, 1); }
    long long pix_lo() const { return dom_.off(0, dom_.y_lo); }
    long long pix_hi() const { return dom_.off(0, dom_.y_hi); }

    void allocate() {
        op_.reset(new Op(spec_, opts_, dom_));
        L_ = op_->layout();
        n_ = L_.off[L_.nimg];
        for (T** v : {&r_, &diag_, &pre_, &p_, &Ap_, &delta_})
            *v = (T*)dmalloc(sizeof(T) * n_);
        if (lm_)
            for (T** v : {&b_, &CtC_, &SSq_, &prev_, &Adelta_})
                *v = (T*)dmalloc(sizeof(T) * n_);
        for (T* v : {r_, diag_, pre_, p_, Ap_, delta_, b_, CtC_, SSq_, prev_, Adelta_})
            if (v) OPT_HIP_CHECK(hipMemset(v, 0, sizeof(T) * n_));
        if constexpr (HasBlockPre<Op>::value) {
            block_ = op_->block_pre();
            if (block_) {
                const long long nb = op_->block_entries();
                blk_ = (T*)dmalloc(sizeof(T) * nb);
                z_ = (T*)dmalloc(sizeof(T) * n_);
                OPT_HIP_CHECK(hipMemset(blk_, 0, sizeof(T) * nb));
                OPT_HIP_CHECK(hipMemset(z_, 0, sizeof(T) * n_));
                op_->set_block_buffer(blk_);
            }
        }
        if constexpr (HasSchur<Op>::value) {
            schur_ = op_->schur();
            if (schur_) {
                const long long ne = op_->schur_entries();
                w_ = (T*)dmalloc(sizeof(T) * ne);
                be_ = (T*)dmalloc(sizeof(T) * ne);
                OPT_HIP_CHECK(hipMemset(w_, 0, sizeof(T) * ne));
                OPT_HIP_CHECK(hipMemset(be_, 0, sizeof(T) * ne));
                op_->set_schur_buffers(w_, be_);
            }
        }
        if constexpr (HasExplicitMatrix<Op>::value) matrix_ = op_->matrix_form();
        flags_ = (uint8_t*)dmalloc(dom_.npix_mem());
        OPT_HIP_CHECK(hipMemset(flags_, 0, dom_.npix_mem()));
        red_.ensure(std::max(op_->stencil_blocks(), 4096), 2, 64);
        if constexpr (HasDumpJ<Op>::value) {
            if (opts_.materialized)
                mat_.reset(new MaterializedJacobian<T>(op_->jacobian_rows(), op_->jacobian_nnz(), n_,
                                                       opts_.fused_jtj));
        }
    }
    void release() {
        drop_graph();
        for (T** v : {&r_, &diag_, &pre_, &p_, &Ap_, &delta_, &b_, &CtC_, &SSq_, &prev_, &Adelta_, &blk_, &z_, &w_, &be_}) {
            dfree(*v);
            *v = nullptr;
        }
        dfree(flags_);
        flags_ = nullptr;
        mat_.reset();
        op_.reset();
    }

    // the stand-alone reduced entry points' preparation: bind, J^T F and its blocks, the
    // scalar init kernel as in step(), then schur_prepare without the right-hand side
    void reduced_prepare(void** params, bool damped = true) {
        prepare(params);
        red_.ensure(std::max(op_->stencil_blocks(), 4096), 4, kScBase + kSlots * (std::max(0, sp_.lIterations) + 2));
        linear_init(kScTmp, false);   // (its flag exchange is idle here: Eliminate refuses row slabs)
        schur_prepare(false, damped);
    }

    // The linear system of a Step at the current unknowns (PCGInit1 + LM's diagonal): r_ = -J^T F,
    // diag(J^T J) and the flags, the neighbours' flags, then pre_, p_0 (LM: b_, CtC_, SSq_ too)
    // and rz_0 into slot `out`. `timed`: step()'s brackets; the stand-alone entry points add
    // nothing to the timer. LM takes the plan's current radius (the parameter's before init)
    // and, until the first step is taken, the FIRST form, which saves SSq (PCGSaveSSq).
    void linear_init(int out, bool timed) {
        const long long lo = pix_lo(), hi = pix_hi();
        const ReduceSlot rs = red_.slot(fg(), out);
        if (timed) tbegin("jtf");
        op_->jtf(r_, diag_, flags_, stream_);
        if (timed) tend();
        exchange({{(void*)flags_, (size_t)dom_.W}});
        if (timed) tbegin(lm_ ? "lm_init" : "gn_init");
        if (!lm_) {
            hipLaunchKernelGGL((gn_init_kernel<T>), dim3(fg()), dim3(kBlock), 0, stream_, L_, (const uint8_t*)flags_,
                               r_, (const T*)diag_, pre_, p_, use_pre(), lo, hi, rs);
        } else {
            LMScalars lm{initialised_ ? radius_ : sp_.trust_region_radius, sp_.min_lm_diagonal, sp_.max_lm_diagonal};
            if (!initialised_ || n_iter_ == 0)
                hipLaunchKernelGGL((lm_init_kernel<T, true>), dim3(fg()), dim3(kBlock), 0, stream_, L_,
                                   (const uint8_t*)flags_, r_, (const T*)diag_, SSq_, CtC_, pre_, b_, p_,
                                   use_pre(), lm, lo, hi, rs);
            else
                hipLaunchKernelGGL((lm_init_kernel<T, false>), dim3(fg()), dim3(kBlock), 0, stream_, L_,
                                   (const uint8_t*)flags_, r_, (const T*)diag_, SSq_, CtC_, pre_, b_, p_,
                                   use_pre(), lm, lo, hi, rs);
        }
        if (timed) tend();
        OPT_HIP_CHECK(hipGetLastError());
    }
    // ---- the assembled matrix of an explicit plan (HasExplicitMatrix) ----
    // the timer entry of a stage: it carries the form's name
    const char* explicit_name(const char* schur, const char* normal) const {
        return matrix_ == MatrixForm::Schur ? schur : normal;
    }
    bool explicit_shape(MatrixForm form, long long* rows, int* dim, long long* nnzb) const {
        if constexpr (HasExplicitMatrix<Op>::value)
            if (matrix_ == form) return op_->matrix_shape(rows, dim, nnzb);
        (void)form; (void)rows; (void)dim; (void)nnzb;
        return false;
    }
    // the matrix at the current unknowns copied out, or (no arrays) bind + pattern only; 1 on a
    // plan without that matrix
    int explicit_matrix(MatrixForm form, void** params, int* rowPtr, int* colInd, void* val) {
        if constexpr (HasExplicitMatrix<Op>::value) {
            if (matrix_ != form) return 1;
            begin_call();
            if (!rowPtr) {
                op_->bind(params, stream_);
                explicit_symbolic();
            } else {
                if (form == MatrixForm::Schur) {
                    reduced_prepare(params);
                } else {
                    prepare(params);
                    op_->jtf(r_, diag_, flags_, stream_);
                    explicit_prepare();
                }
                op_->matrix_copy(rowPtr, colInd, (T*)val, stream_);
            }
            end_call();
            return 0;
        }
        (void)form; (void)params; (void)rowPtr; (void)colInd; (void)val;
        return 1;
    }
    // the pattern for the graphs as bound (a no-op while the wiring stands). A rebuild moves the
    // SpMV's buffers, so no captured loop survives it.
    void explicit_symbolic() {
        if constexpr (HasExplicitMatrix<Op>::value)
            if (matrix_ != MatrixForm::None && op_->matrix_symbolic_stale()) {
                drop_graph();
                tbegin(explicit_name("schur_symbolic", "normal_symbolic"));
                op_->matrix_symbolic(stream_);
                tend();
            }
    }
    // ... and the matrix itself from the blocks in blk_, before block_init inverts them
    void explicit_prepare() {
        if constexpr (HasExplicitMatrix<Op>::value)
            if (matrix_ != MatrixForm::None) {
                explicit_symbolic();
                tbegin(explicit_name("schur_eblk", "normal_eblk")); op_->matrix_eblk(stream_); tend();
                tbegin(explicit_name("schur_assemble", "normal_assemble")); op_->matrix_assemble(stream_); tend();
            }
    }
    // Ap = S p or H p (+ dadd p) by the block SpMV; false on any other plan
    bool explicit_apply(const T* p, T* Ap, const T* dadd, const int* stop, ReduceSlot rs) {
        if constexpr (HasExplicitMatrix<Op>::value)
            if (matrix_ != MatrixForm::None) {
                tbegin(explicit_name("schur_spmv", "normal_spmv")); op_->matrix_spmv(p, Ap, dadd, stop, rs, stream_); tend();
                return true;
            }
        (void)p; (void)Ap; (void)dadd; (void)stop; (void)rs;
        return false;
    }

    // LinearSolver("cholesky") (HasExplicitMatrix, Op::direct_solver): in place of the PCG loop, the
    // assembled matrix (+ LM's diagonal) filled into dense tiles with the retained part of r_ as
    // the right-hand side, factored and solved into delta_ (dense_cholesky.h). false, with delta_
    // untouched, where the plan has no such statement, Lit = 0, the storage does not fit
    // (OPT_AMD_DENSE_MAX_BYTES, default 2 GiB, or the free device memory) or a pivot fails: the
    // caller then runs the PCG loop, for which everything up to block_init has been done as ever.
    // The host reads the failure flag once after the factorisation: one 16-byte copy and one
    // stream sync per Step.
    bool direct_step(int Lit) {
        if constexpr (HasExplicitMatrix<Op>::value)
            if (matrix_ != MatrixForm::None && op_->direct_solver() && Lit > 0) {
                long long rows = 0, nnzb = 0;
                int dim = 0;
                if (!op_->matrix_shape(&rows, &dim, &nnzb) || rows * dim < 1) return false;
                const long long n = rows * dim;
                direct_n_ = n;
                {   // the cap is read at every Step; the free memory counts only while nothing is allocated
                    const char* cap = getenv("OPT_AMD_DENSE_MAX_BYTES");
                    const unsigned long long max_bytes = cap && *cap ? strtoull(cap, nullptr, 10) : (2ULL << 30);
                    const size_t need = dense_bytes(n, sizeof(T));
                    bool fits = need <= max_bytes;
                    if (fits && dense_.n() != n) {
                        dense_.release();
                        size_t free_b = 0, total_b = 0;
                        OPT_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
                        fits = need <= free_b;
                    }
                    if (!fits) {
                        dense_.release();
                        ++direct_fallbacks_;
                        direct_reason_ = "memory";
                        return false;
                    }
                    dense_.resize(n);
                }
                tbegin("dense_fill");
                OPT_HIP_CHECK(hipMemsetAsync(dense_.tiles(), 0, sizeof(T) * (size_t)dense_tile_count(n) * kDenseNB * kDenseNB, stream_));
                dense_.reset(stream_);
                op_->dense_fill(lm_ ? CtC_ : nullptr, r_, dense_.tiles(), dense_.diag0(), dense_.rhs(), stream_);
                tend();
                tbegin("dense_factor"); dense_.factor(stream_); tend();
                double ratio = INFINITY;
                if (dense_.status(stream_, &ratio) >= 0) {   // (min_pivot_ratio stays the last completed factorisation's)
                    ++direct_fallbacks_;
                    direct_reason_ = "pivot";
                    return false;
                }
                direct_ratio_ = ratio;
                tbegin("dense_solve");
                dense_.solve(stream_);
                op_->dense_store(dense_.solution(), delta_, &dense_.status_dev()->fail, stream_);
                tend();
                ++direct_factorisations_;
                return true;
            }
        (void)Lit;
        return false;
    }
    // covariance() between begin_call and end_call (HasExplicitMatrix plans with the statement)
    int covariance_body(void** params, long long nPairs, const int* rowElem, const int* colElem, T* blocks, std::string* why) {
        if (matrix_ == MatrixForm::Schur) {
            reduced_prepare(params, false);
        } else {
            prepare(params);
            op_->jtf(r_, diag_, flags_, stream_);
            explicit_prepare();
        }
        long long rows = 0, nnzb = 0;
        int dim = 0;
        if (!op_->matrix_shape(&rows, &dim, &nnzb) || rows * dim < 1) return *why = "covariance: the plan's matrix is empty", -1;
        const long long n = rows * dim;
        DenseSelection sel;
        if (nPairs < 0 || (nPairs > 0 && (!rowElem || !colElem || !blocks)) || !sel.build(n, dim, nPairs, rowElem, colElem))
            return *why = "covariance: NULL array or element out of range (the matrix has " + std::to_string(rows) + " block rows)", -1;
        {   // tiles + workspace against the cap, read at every call, and what is still to allocate against the free memory
            const char* cap = getenv("OPT_AMD_DENSE_MAX_BYTES");
            const unsigned long long max_bytes = cap && *cap ? strtoull(cap, nullptr, 10) : (2ULL << 30);
            const size_t tiles = dense_bytes(n, sizeof(T)), ws = dense_cov_bytes(sel, sizeof(T));
            bool fits = tiles + ws <= max_bytes;
            if (fits) {
                size_t free_b = 0, total_b = 0;
                OPT_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
                const size_t have = dense_.n() == n ? tiles + (dense_.cov_capacity() == ws ? ws : 0) : 0;
                const size_t freed = dense_.n() == n ? (dense_.cov_capacity() == ws ? 0 : dense_.cov_capacity())
                                                     : (dense_.n() ? dense_bytes(dense_.n(), sizeof(T)) + dense_.cov_capacity() : 0);
                fits = tiles + ws - have <= free_b + freed;
            }
            if (!fits)
                return *why = "covariance: reason=memory: tiles " + std::to_string(tiles) + " + workspace " + std::to_string(ws) +
                              " bytes exceed OPT_AMD_DENSE_MAX_BYTES or the free device memory", 2;
            dense_.resize(n);
            direct_n_ = n;
            cov_bytes_ = (long long)ws;
        }
        tbegin("cov_fill");
        OPT_HIP_CHECK(hipMemsetAsync(dense_.tiles(), 0, sizeof(T) * (size_t)dense_tile_count(n) * kDenseNB * kDenseNB, stream_));
        dense_.reset(stream_);
        hipLaunchKernelGGL((fill_kernel<T>), dim3(fg()), dim3(kBlock), 0, stream_, n_, (T)1, Ap_);
        op_->dense_fill(nullptr, Ap_, dense_.tiles(), dense_.diag0(), dense_.rhs(), stream_);
        tend();
        tbegin("cov_factor"); dense_.factor(stream_); tend();
        const int fail = dense_.status(stream_, nullptr);
        if (fail >= 0)
            return *why = "covariance: reason=pivot row=" + std::to_string(fail) + " element=" + std::to_string(fail / dim) +
                          " channel=" + std::to_string(fail % dim) + ": the matrix is singular there (gauge freedom?)", 3;
        tbegin("cov_forward");
        dense_.cov_begin(sel, stream_);
        dense_.cov_forward(sel, stream_);
        tend();
        tbegin("cov_gram"); dense_.cov_gram(sel, dense_.rhs(), blocks, stream_); tend();
        ++covariances_;
        return 0;
    }

    // Schur plans, after the scalar init kernel and before block_init: M_e^-1 in place of the
    // eliminated blocks, b_e stashed and cleared, 1/2 b_e.M^-1 b_e beside q0 (gen_blk_step2's exit
    // test adds it); with `rhs` also r_r -= E M^-1 b_e (b_ too in LM) through one reduced apply
    // of p = 0 — the caller's delta_, zeroed at the start of the step. `damped` = false leaves LM's
    // diagonal out of M_e too (covariance(): the undamped S).
    void schur_prepare(bool rhs, bool damped = true) {
        if constexpr (HasSchur<Op>::value)
            if (schur_) {
                tbegin("schur_rhs");
                op_->schur_rhs(CtC_, r_, b_, lm_ && damped ? 1 : 0, red_.slot(nb(), kScQc), stream_);
                if (rhs) {
                    op_->schur_apply(delta_, Ap_, nullptr, nullptr, red_.slot(nb(), kScTmp), stream_);
                    hipLaunchKernelGGL((schur_sub_kernel<T>), dim3(fg()), dim3(kBlock), 0, stream_, n_, r_, (const T*)Ap_,
                                       lm_ ? b_ : nullptr);
                    OPT_HIP_CHECK(hipGetLastError());
                }
                tend();
                if (matrix_ == MatrixForm::Schur) explicit_prepare();   // S itself: M_e^-1 is in blk, B_r not yet inverted
            }
    }
    // the reduced apply Ap = S p (two launches; an explicit plan's is explicit_apply); false on
    // a plan without Eliminate
    bool schur_apply(const T* p, T* Ap, const T* dadd, const int* stop, ReduceSlot rs) {
        if (matrix_ == MatrixForm::Schur) return explicit_apply(p, Ap, dadd, stop, rs);
        if constexpr (HasSchur<Op>::value)
            if (schur_) {
                tbegin("schur_elim"); op_->schur_elim(p, stream_); tend();
                tbegin("schur_apply"); op_->schur_apply(p, Ap, dadd, stop, rs, stream_); tend();
                return true;
            }
        (void)p; (void)Ap; (void)dadd; (void)stop; (void)rs;
        return false;
    }

    // ---- the stages of one PCG iteration (pcg_loop, pcg_loop_fused): each picks its variant
    // and returns. Slots of iteration i: rz(i), pap(i) in, rz(i + 1) / q(i + 1) out.
    int use_pre() const { return spec_.use_preconditioner ? 1 : 0; }
    ZetaArgs zeta_args(int i) const {
        return ZetaArgs{red_.scalars + kScQ0, stop_, i, sp_.q_tolerance, (lm_ && !distributed()) ? 1 : 0};
    }
    bool reset_iteration(int i) const { return lm_ && ((i + 1) % std::max(1, sp_.residual_reset_period)) == 0; }
    // the apply as interior + boundary launches around the halo refresh of p
    bool halo_split() const {
        if constexpr (HasApplySplit<Op>::value)
            return distributed() && overlap_ && comm_->concurrent_halo() && !mat_ && op_->can_split();
        return false;
    }
    // PCGStep3 folded into the next apply (HasFusedStep3). Never on a block plan: tested here,
    // before step3_fused and apply_prepared are, so the block stages' z is not bypassed.
    bool fuse3() const {
        if constexpr (HasFusedStep3<Op>::value) return !distributed() && !mat_ && !block_ && fuse3_on_;
        return false;
    }
    // GN with step3_kernel: the delta update rides in PCGStep3 (reads p_old anyway)
    bool delta3() const { return !lm_ && delta3_on_ && !fuse3(); }

    // PCGStep1: Ap_ = A p_ and p.Ap into pap(i), by the first variant that holds. Only the
    // split variant refreshes p's halo itself; every other one needs it done before.
    void pcg_apply(int i, const int* stop) {
        const T* dadd = lm_ ? CtC_ : nullptr;
        const ReduceSlot rs = red_.slot(nb(), pap(i));
        if constexpr (HasApplySplit<Op>::value)
            if (halo_split()) {
                // halo refresh of p beside the interior blocks (Plan::halo_mark/begin/join)
                tbegin(Op::kApplyName);
                halo_mark();
                op_->apply_split(1, p_, Ap_, dadd, stop, rs, stream_);
                halo_begin(comm_, vec_planes(p_), dom_, op_->halo());
                halo_join();
                op_->apply_split(2, p_, Ap_, dadd, stop, rs, stream_);
                tend();
                return;
            }
        exchange_vec(p_);
        if (mat_) {
            // cusparseInner + PCGStep1_Finish (:2101-2118): the SpMV replaces PCGStep1;
            // as in the reference, the LM CtC term is not part of this product
            mat_apply(p_, Ap_, stop, pap(i));
            return;
        }
        if constexpr (HasFusedStep3<Op>::value)
            if (i > 0 && fuse3()) {   // step3 of i-1 already ran the apply's first pass
                tbegin(Op::kApplyName);
                op_->apply_prepared(p_, Ap_, dadd, stop, rs, stream_);
                tend();
                return;
            }
        if constexpr (HasApplyExt<Op>::value) {
            hipEvent_t e0 = nullptr, e1 = nullptr;
            if (timer_.mode && timer_.ext_pair(Op::kApplyName, &e0, &e1)) {
                op_->apply_ext(p_, Ap_, dadd, stop, rs, stream_, e0, e1);
                timer_.ext_record(Op::kApplyName, e0, e1);
                return;
            }
        }
        if (schur_apply(p_, Ap_, dadd, stop, rs)) return;
        if (explicit_apply(p_, Ap_, dadd, stop, rs)) return;
        tbegin(Op::kApplyName);
        op_->apply(p_, Ap_, dadd, stop, rs, stream_);
        tend();
    }
    // the fused loop's PCGStep1: the apply with its four sums (HasApplySums) into pap(i) and the
    // three slots after it, split around the halo refresh of p where pcg_apply would be
    void pcg_apply_sums(int i, const int* stop) {
        const T* w = use_pre() ? pre_ : nullptr;   // PCGStep2's weighting W (1 without a preconditioner)
        const ReduceSlot rs = red_.slot(nb(), pap(i));
        auto launch = [&](int part) {
            hipEvent_t e0 = nullptr, e1 = nullptr;
            const bool ev = part == 0 && timer_.mode && timer_.ext_pair(Op::kApplyName, &e0, &e1);
            if (!ev) tbegin(Op::kApplyName);
            op_->apply_sums(part, p_, Ap_, lm_ ? CtC_ : nullptr, stop, rs, r_, w, stream_, e0, e1);
            if (ev) timer_.ext_record(Op::kApplyName, e0, e1);
            else tend();
        };
        if (halo_split()) {
            halo_mark();
            launch(1);
            halo_begin(comm_, vec_planes(p_), dom_, op_->halo());
            halo_join();
            launch(2);
        } else {
            exchange_vec(p_);
            launch(0);
        }
    }
    // PCGStep2: alpha, delta += alpha p (unless it rides in step3), r -= alpha Ap, z, rz / q
    void pcg_step2(int i, const int* stop, const ZetaArgs& z) {
        if constexpr (HasBlockPre<Op>::value)
            if (block_) {
                tbegin("blk_step2");
                op_->block_step2(p_, Ap_, b_, r_, delta_, z_, red_.scalars, rz(i), pap(i), i == 0 ? 1 : 0,
                                 lm_ ? 1 : 0, (lm_ || !delta3()) ? 1 : 0, stop, red_.slot(nb(), rz(i + 1)), z, stream_);
                tend();
                return;
            }
        tbegin("step2");
        launch_step2(i == 0, rz(i), pap(i), rz(i + 1), stop, z, !delta3());
        tend();
    }
    // PCGStep2 + PCGStep3 as one pass (the fused loop)
    void pcg_step23(int i, const int* stop, const ZetaArgs& z) {
        tbegin("step23");
        const ReduceSlot rs2 = red_.slot(fg(), rz(i + 1));
#define S23(F, L)                                                                                              \
    hipLaunchKernelGGL((step23_kernel<T, F, L>), dim3(fg()), dim3(kBlock), 0, stream_, n_, p_, (const T*)Ap_,      \
                       (const T*)pre_, (const T*)b_, r_, delta_, red_.scalars, rz(i), rz(i + 1) + 6, use_pre(), stop, rs2, \
                       z)
        if (i == 0 && lm_) S23(true, true);
        else if (lm_) S23(false, true);
        else if (i == 0) S23(true, false);
        else S23(false, false);
#undef S23
        OPT_HIP_CHECK(hipGetLastError());
        tend();
    }
    // A residual-reset iteration (LM) in place of step2: delta += alpha p, then r = b - A delta
    // from an apply of delta itself (always matrix-free, unsplit and untimed), z, rz / q.
    // GUARD: the fused loop's form of the division, as step23_kernel has it.
    template <bool GUARD>
    void pcg_half1(int i, const int* stop) {
        hipLaunchKernelGGL((half1_kernel<T, GUARD>), dim3(fg()), dim3(kBlock), 0, stream_, n_, (const T*)p_, delta_,
                           red_.scalars, rz(i), pap(i), stop);
    }
    void pcg_reset_apply(const int* stop) {
        exchange_vec(delta_);
        if (!schur_apply(delta_, Adelta_, CtC_, stop, red_.slot(nb(), kScTmp)) &&
            !explicit_apply(delta_, Adelta_, CtC_, stop, red_.slot(nb(), kScTmp)))
            op_->apply(delta_, Adelta_, CtC_, stop, red_.slot(nb(), kScTmp), stream_);
    }
    void pcg_half2(int i, const int* stop, const ZetaArgs& z) {
        if constexpr (HasBlockPre<Op>::value)
            if (block_) {
                tbegin("blk_half2");
                op_->block_half2(Adelta_, b_, delta_, r_, z_, stop, red_.slot(nb(), rz(i + 1)), z, stream_);
                tend();
                return;
            }
        hipLaunchKernelGGL((half2_kernel<T>), dim3(fg()), dim3(kBlock), 0, stream_, n_, (const T*)Adelta_,
                           (const T*)b_, (const T*)pre_, (const T*)delta_, r_, use_pre(), stop,
                           red_.slot(fg(), rz(i + 1)), z);
    }
    // PCGStep3 folded into the Op's next apply; false where there is no such thing
    bool pcg_step3_fused(int i, const int* stop) {
        if constexpr (HasFusedStep3<Op>::value)
            if (fuse3()) {
                tbegin("step3");
                op_->step3_fused(pre_, r_, p_, red_.scalars, rz(i + 1), rz(i), use_pre(), stop, stream_);
                tend();
                return true;
            }
        (void)i; (void)stop;
        return false;
    }
    // PCGStep3: p = z + beta p, on the block stages' z_ as it is, else on pre_ r_ (or r_); with
    // delta3() also GN's delta update, written at i = 0 and added to after. GUARD (the fused
    // loop's reset iterations, LM: no delta here) as for pcg_half1.
    template <bool GUARD>
    void pcg_step3(int i, const int* stop) {
        const T* zs = block_ ? z_ : r_;
        const int up = block_ ? 0 : use_pre();
        const int dm = delta3() ? (i == 0 ? 1 : 2) : 0;
        tbegin("step3");
#define S3(DM)                                                                                                   \
    hipLaunchKernelGGL((step3_kernel<T, DM, GUARD>), dim3(fg()), dim3(kBlock), 0, stream_, n_, (const T*)pre_, zs, p_, \
                       red_.scalars, rz(i + 1), rz(i), up, stop, DM ? delta_ : nullptr, DM ? rz(i) : 0,          \
                       DM ? pap(i) : 0)
        if constexpr (GUARD) S3(0);
        else if (dm == 1) S3(1);
        else if (dm == 2) S3(2);
        else S3(0);
#undef S3
        tend();
    }
    // LM's exit test on q(i + 1) as its own launch, where no kernel carries it (ZetaArgs::on == 0)
    void pcg_zeta(int i) {
        hipLaunchKernelGGL((zeta_kernel<T>), dim3(1), dim3(1), 0, stream_, red_.scalars, q(i + 1),
                           red_.scalars + kScQ0, i, sp_.q_tolerance, stop_);
    }

    // bind + unknown halo + ComputedArrays, for the standalone entry points
    void prepare(void** params) {
        op_->bind(params, stream_);
        exchange_unknowns();
        op_->precompute(stream_);
        exchange_computed();
        loss_weights();
    }
    void precompute() {
        tbegin("precompute"); op_->precompute(stream_); tend();
        exchange_computed();
        loss_weights();
    }
    // robust losses: the per-edge weights of this linearisation (HasLossWeights)
    void loss_weights() {
        if constexpr (HasLossWeights<Op>::value)
            if (op_->has_loss()) {
                tbegin("gen_loss_weights"); op_->loss_weights(stream_); tend();
            }
    }

    bool distributed() const { return comm_ && comm_->size() > 1; }
    void allreduce(int idx, int n) {
        if (distributed()) comm_->allreduce_sum(red_.scalars + idx, n, stream_);
    }
    void exchange(const std::vector<HaloPlane>& planes) {
        if (!distributed() || planes.empty()) return;
        tbegin("halo_exchange");
        comm_->halo_exchange(planes, dom_, op_->halo(), stream_);
        tend();
    }
    std::vector<HaloPlane> vec_planes(T* v) const {
        std::vector<HaloPlane> pl;
        for (int k = 0; k < L_.nimg; ++k) pl.push_back({(void*)(v + L_.off[k]), sizeof(T) * L_.ch[k] * dom_.W});
        return pl;
    }
    void exchange_vec(T* v) {
        if (!distributed()) return;
        exchange(vec_planes(v));
    }
    void exchange_unknowns() {
        if (!distributed()) return;
        std::vector<HaloPlane> pl;
        for (int k = 0; k < L_.nimg; ++k) pl.push_back({(void*)op_->unknown(k), sizeof(T) * L_.ch[k] * dom_.W});
        exchange(pl);
    }
    void exchange_computed() {
        if (!distributed()) return;
        std::vector<HaloPlane> pl;
        op_->computed_planes(pl);
        exchange(pl);
    }

    void launch_step2(bool first, int i_num, int i_den, int out, const int* stop, ZetaArgs z = {},
                      bool delta = true) {
        const int g = fg();
        auto slot = red_.slot(g, out);
#define S2(F, LMV, D)                                                                                  \
    hipLaunchKernelGGL((step2_kernel<T, F, LMV, D>), dim3(g), dim3(kBlock), 0, stream_, n_, (const T*)p_, \
                       (const T*)Ap_, (const T*)pre_, (const T*)b_, r_, delta_, red_.scalars, i_num,    \
                       i_den, use_pre(), stop, slot, z)
        if (first && lm_) S2(true, true, true);
        else if (lm_) S2(false, true, true);
        else if (!delta) S2(false, false, false);
        else if (first) S2(true, false, true);
        else S2(false, false, true);
#undef S2
    }
    UnknownPtrs<T> unknowns() {
        UnknownPtrs<T> X{};
        for (int k = 0; k < L_.nimg && k < 4; ++k) X.x[k] = op_->unknown(k);
        return X;
    }
    void update(bool save) {
        tbegin("update");
        if (save)
            hipLaunchKernelGGL((update_images_kernel<T, true>), dim3(fg()), dim3(kBlock), 0, stream_, L_,
                               (const uint8_t*)flags_, unknowns(), (const T*)delta_, prev_,
                               pix_lo(), pix_hi());
        else
            hipLaunchKernelGGL((update_images_kernel<T, false>), dim3(fg()), dim3(kBlock), 0, stream_, L_,
                               (const uint8_t*)flags_, unknowns(), (const T*)delta_, prev_,
                               pix_lo(), pix_hi());
        OPT_HIP_CHECK(hipGetLastError());
        tend();
        exchange_unknowns();
    }
    void revert() {
        hipLaunchKernelGGL((revert_images_kernel<T>), dim3(fg()), dim3(kBlock), 0, stream_, L_,
                           (const uint8_t*)flags_, unknowns(), (const T*)prev_, pix_lo(),
                           pix_hi());
        OPT_HIP_CHECK(hipGetLastError());
        exchange_unknowns();
    }
    // J at the current unknowns (saveJToCRS), then J^T (+ J^T J) values (cusparseOuter)
    void materialize() {
        if constexpr (HasDumpJ<Op>::value) {
            if constexpr (HasTopologyGeneration<Op>::value) {
                // a re-wired graph: patterns of the old wiring are in range but wrong; their
                // buffers and the apply's grid change, so no captured loop survives either
                const unsigned long long gen = op_->topology_generation();
                if (gen != mat_generation_) {
                    mat_->drop_patterns();
                    drop_graph();
                    mat_generation_ = gen;
                }
            }
            tbegin("saveJToCRS");
            op_->dump_j(mat_->rowPtrJ(), mat_->colIndJ(), mat_->valJ(), stream_);
            tend();
            mat_->build([this](const char* n, bool b) { if (b) tbegin(n); else tend(); }, stream_);
        }
    }
    void mat_apply(const T* p, T* Ap, const int* stop, int out) {
        PcgMask m{L_, (const uint8_t*)flags_, pix_lo(), pix_hi(), stop};
        mat_->apply(p, Ap, m, red_.slot(mat_->blocks(), out), [this](const char* n, bool b) {
            if (b) tbegin(n); else tend();
        }, stream_);
    }
    double read(int idx) { return read_device_scalar(red_.scalars + idx); }

    Domain dom_;
    std::unique_ptr<Op> op_;
    Comm* comm_ = nullptr;
    bool lm_ = false;
    VecLayout L_;
    long long n_ = 0;
    T *r_ = nullptr, *diag_ = nullptr, *pre_ = nullptr, *p_ = nullptr, *Ap_ = nullptr, *delta_ = nullptr;
    T *b_ = nullptr, *CtC_ = nullptr, *SSq_ = nullptr, *prev_ = nullptr, *Adelta_ = nullptr;
    bool block_ = false;                       // block preconditioner (HasBlockPre)
    T *blk_ = nullptr, *z_ = nullptr;          // its blocks (inverted in place) and z = M^-1 r
    bool schur_ = false;                       // Eliminate: PCG on the Schur complement (HasSchur)
    T *w_ = nullptr, *be_ = nullptr;           // compact (eliminated elements): M^-1-sized products, the stash of b_e
    DenseFactor<T> dense_;                     // LinearSolver("cholesky"): the tiles, allocated at the first direct Step
    long long direct_n_ = 0, direct_factorisations_ = 0, direct_fallbacks_ = 0;
    long long covariances_ = 0, cov_bytes_ = 0;   // covariance(): calls completed, the last workspace
    double direct_ratio_ = INFINITY;
    const char* direct_reason_ = "none";
    MatrixForm matrix_ = MatrixForm::None;     // S or H assembled per step, the apply a block SpMV (HasExplicitMatrix)
    uint8_t* flags_ = nullptr;
    int* stop_ = nullptr;
    hipGraphExec_t graph_exec_ = nullptr;      // captured PCG loop (pcg_graph_begin)
    std::vector<unsigned long long> graph_key_;
    bool capturing_ = false;
    const bool graph_off_ = getenv("OPT_AMD_NO_GRAPH") && atoi(getenv("OPT_AMD_NO_GRAPH"));
    const bool overlap_ = env_int("OPT_AMD_HALO_OVERLAP", 1) != 0;   // 0: blocking halo before each apply
    const bool fuse3_on_ = env_int("OPT_AMD_FUSE_STEP3", 1) != 0;   // 0: step3_kernel + the whole apply
    // Ops with apply_sums: OPT_AMD_FUSE23=0 the classic apply / step2 / step3 loop, 1 the
    // fused loop, 2 (default) the fused loop on row slabs only. One GPU, shape_from_shading
    // 4096^2 LM: the apply with the four sums takes 175 us against 131 (r read back, 6
    // instead of 7 waves per SIMD), more than step3's pass saves: 3.56 vs 3.36 ms per step
    // (tools/history/r03_fuse23.sh). On slabs the fused loop saves an all-reduce per iteration.
    const int fuse23_ = env_int("OPT_AMD_FUSE23", 2);
    const bool delta3_on_ = env_int("OPT_AMD_DELTA_IN_STEP3", 1) != 0;   // 0: delta updated by step2
    std::unique_ptr<MaterializedJacobian<T>> mat_;
    unsigned long long mat_generation_ = 0;    // Op::topology_generation() mat_'s patterns were built for
    float radius_ = 1e4f, decrease_ = 2.0f;
};

// Plan factory for the generic driver: refuses useMaterializedJTJ for a family without
// a J assembly (the reference returns a nil plan on compile errors, o.t:1352,1526).
template <class Op>
std::unique_ptr<Plan> make_stencil_plan(const ProblemSpec& spec, const StateOptions& opts, Domain dom,
                                        std::string* err) {
    if (opts.materialized && !HasDumpJ<Op>::value) {
        *err = std::string(Op::kName) + ": no materialized Jacobian (useMaterializedJTJ) for this energy family";
        return nullptr;
    }
    return std::unique_ptr<Plan>(new StencilPlan<Op>(spec, opts, dom));
}

}  // namespace optamd
