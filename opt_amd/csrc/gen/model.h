// gen/model.h — an energy file lowered to declarations + scalar residual templates.
//
// The reference runs the energy file as a Lua program against lib.t / ProblemSpecAD
// (API/src/o.t:1295-1348) and turns every Energy term into residual templates grouped by
// domain (toenergyspecs / classifyexpression, o.t:2669-2715). build_model() does the same
// with a Lua-subset interpreter (gen/lua.cpp): the result lists the declarations in
// problemparams order and one template per scalar residual, each with its domain
// (centred over the unknowns' index space, or a graph) and its unknown support.
#pragma once
#include <string>
#include <vector>
#include "ir.h"

namespace optamd {
namespace gen {

struct GDim { std::string name; int index = -1; };
struct GImage {
    std::string name;
    int index = -1;              // position in problemparams
    int channels = 1;
    bool unknown = false;
    std::vector<int> dims;       // GDim ids
    std::string elem = "float";  // element type of a known array ("float", "uint8", ...)
    int space = -1;              // GModel::spaces id of dims (build_model fills it)
    bool internal = false;       // ComputedArray value / gradient image: allocated by the plan
    bool tvalued = false;        // stored in the solver precision T (unknowns, internal
                                 // images, arrays aliasing an unknown's parameter slot)
};
// d(computed channel)/d(unknown access u): a gradient image (gimg) or a constant (gimg -1)
struct GGrad { int ch = 0; int u = -1; int expr = -1; int gimg = -1; };
// ComputedArray (ProblemSpecAD:ComputedImage, o.t:1686-1718): evaluated per pixel by the
// precompute kernel (createprecomputed, o.t:3131-3153) with its gradient images.
struct GComputed {
    int image = -1;
    std::vector<int> expr;         // per channel
    std::vector<GGrad> grads;
    int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};   // bbox of the expression (bboxforexpression)
    bool per_step = false;         // a private cache of bound arrays (lua.cpp cache_samples),
                                   // not a ComputedArray of the energy: also rebuilt at Step start
    int space = -1;                // index space of its image
};
struct GParam { std::string name; std::string type; int index = -1; };
struct GGraph {
    std::string name;
    std::vector<int> dims;                // edge-count GDim ids
    std::vector<std::string> slot_names;
    std::vector<int> slot_index;          // problemparams index of each vertex array
    std::vector<std::vector<int>> slot_dims;   // the index space each slot's vertices lie in (GDim ids)
    std::vector<int> slot_space;          // its GModel::spaces id
};
struct GResidual {
    int expr = -1;                 // scalar expression (centred: wrapped in its bbox select)
    int graph = -1;                // -1: centred over the unknowns' index space
    std::vector<int> unknowns;     // distinct unknown Read nodes (the support)
    int space = -1;                // centred: the index space it is instantiated over
};

// A block group of the block preconditioner: one index space that holds unknowns; its
// unknown images in problemparams order, each with the block row of its first channel.
struct GBlockGroup {
    int space = -1;
    int C = 0;                     // channels of all its unknown images
    std::vector<int> images;       // image ids
    std::vector<int> first_row;    // per image: row of its channel 0 inside the C x C block
    int entries() const { return C * (C + 1) / 2; }   // packed lower triangle
};

// RobustEnergy(kind, scale, term, ...): one loss block per edge of `graph` over the statement's
// scalar residuals f_1..f_R, s = sum f_k^2. Its templates in GModel::residuals are the
// weighted f~_k = W f_k (W: Pool::weight(group), the cached sqrt(rho'(s)) of the edge), so
// every emitter that differentiates a residual gets the reweighted problem; `raw` keeps the
// f_k for the kernels that need s and rho (gen_cost, gen_loss_weights).
struct GLossGroup {
    enum Kind { Huber = 0, Cauchy = 1 };
    int graph = -1;
    int kind = Huber;
    double scale = 0.0;            // the constant a (scale_param < 0)
    int scale_param = -1;          // GModel::params id of a float Param scale, re-read per evaluation
    std::vector<int> residuals;    // ids in GModel::residuals (the weighted templates), statement order
    std::vector<int> raw;          // the f_k, same order
};

struct GModel {
    Pool pool;
    std::vector<GDim> dims;
    std::vector<GImage> images;
    std::vector<GParam> params;
    std::vector<GGraph> graphs;
    std::vector<GResidual> residuals;
    std::vector<GComputed> computed;   // declaration order (= precompute order)
    int exclude = -1;              // Exclude(expr): centred scalar, -1 = none (the first one declared)
    // Index spaces (the reference's IndexSpace, o.t:548-600): every distinct ordered Dim list
    // an Unknown, Array, ComputedArray or graph slot is declared over, in declaration order.
    // One space: the single-domain energies every kernel form serves. Several: unknowns and
    // arrays of different sizes (cameras / points / observations); centred residuals are
    // instantiated over their own space, graph slots index theirs.
    std::vector<std::vector<int>> spaces;
    std::vector<std::pair<int, int>> excludes;   // (space, expr): at most one Exclude per space
    bool use_preconditioner = false;
    // UsePreconditioner("block"): PCG preconditioned with the inverse of each element's
    // diagonal block of J^T J over all unknown channels of its index space
    bool block_preconditioner = false;
    // Eliminate(X, ...): the unknown images of one index space whose diagonal blocks of J^T J
    // decouple (no residual reads two of its elements); PCG then runs on the Schur complement
    // over the other spaces (build_model checks the group, turns the block preconditioner on)
    std::vector<int> eliminated;   // image ids, unknown_images() order
    int elim_space = -1;           // their space, -1 = no Eliminate
    // ReducedSystem("explicit") beside Eliminate: S is assembled once per step in block-CSR and
    // PCG's apply is a block SpMV (codegen_schur_explicit.cpp); "implicit" / no statement: the
    // matrix-free apply. The shapes this form takes: explicit_refusal()
    bool reduced_explicit = false;
    // NormalMatrix("explicit"): H = J^T J is assembled once per step in block-CSR and PCG's apply
    // is a block SpMV (codegen_normal.cpp); "matrix_free" / no statement: the gather apply. Turns
    // the block preconditioner on. The shapes this form takes: normal_refusal()
    bool normal_explicit = false;
    // LinearSolver("cholesky") beside one of the two explicit statements: the Step's linear system
    // is the assembled matrix, filled into dense tiles, factored and solved (dense_cholesky.h,
    // codegen_dense.cpp) instead of iterated on; "pcg" / no statement: the PCG loop
    bool direct_cholesky = false;
    std::vector<GLossGroup> loss;  // RobustEnergy statements, in order (at most kMaxLossGroups)
    static constexpr int kMaxLossGroups = 4;
    int loss_group_of(int residual) const {   // the group a residual template belongs to, -1 = plain
        for (size_t g = 0; g < loss.size(); ++g)
            for (int r : loss[g].residuals)
                if (r == residual) return (int)g;
        return -1;
    }
    bool schur() const { return elim_space >= 0; }
    bool is_eliminated(int image) const {
        for (int k : eliminated)
            if (k == image) return true;
        return false;
    }
    std::string unsupported;      // first construct the generic path cannot lower
    int n_params_total = 0;

    int unknown_dims() const;      // dimensionality of the (first) unknowns' index space
    bool multi() const { return spaces.size() > 1; }
    int space_of(const std::vector<int>& dims);          // id of dims, registered on first use
    int exclude_of(int space) const;                     // Exclude expression of a space, -1 = none
    std::vector<int> unknown_spaces() const;             // spaces holding unknowns, in unknown_images() order
    std::vector<int> unknown_images() const;   // image ids of the unknowns, declaration order
    std::vector<GBlockGroup> block_groups() const;       // in unknown_spaces() order
};

// Why ReducedSystem("explicit") cannot serve this model ("" = it can): the retained unknowns
// must lie over one index space and B, their block of J^T J, must be block-diagonal (lua.cpp).
std::string explicit_refusal(const GModel& m);
// Why NormalMatrix("explicit") cannot serve this model ("" = it can): all unknowns must lie over
// one index space and every centred term must read them at offset 0, so that the diagonal
// blocks plus the graphs' instance pairs are all of J^T J (lua.cpp).
std::string normal_refusal(const GModel& m);

// Run `text` (an Opt energy file). false + message on a Lua or DSL error.
bool build_model(const std::string& text, GModel* m, std::string* err);

}  // namespace gen
}  // namespace optamd
