// gen/codegen.h — HIP source for a lowered energy (the role of the reference's
// createjtfcentered / createjtjcentered / createjtfgraph / createjtjgraph / createcost /
// createmodelcost, o.t:2770-3129, and of the Terra emitter, o.t:1949-2665).
#pragma once
#include <string>
#include <vector>
#include "model.h"

// Kernel argument block shared by the host (generic.hip) and the generated source: the
// macro bodies are compiled on the host and pasted, stringised, into the generated code.
// The per-space tail is pasted only for energies over several index spaces (GModel::multi):
// a single-space energy's kernels declare, and the runtime copies, the head alone.
// An energy with a RobustEnergy statement pastes both tails (the loss tail follows the spaces'
// on the host); every other energy's argument block, and with it its source, is unchanged.
#define OPTAMD_GENARGS_FIELDS                                                               \
        int dims[3];                /* unknowns' index space, unused dims = 1 */            \
        long long npix;             /* elements of that space */                            \
        const void* img[16];        /* by image id: unknowns (T) and known arrays */        \
        double prm[32];             /* by parameter id, at full width (cast to T on use) */ \
        const int* slot[16];        /* graph vertex arrays, graph-major */                  \
        const int* goff[16];        /* per slot: incidence offsets by vertex (N+1) */       \
        const int* geid[16];        /* per slot: incident edge ids, ascending */            \
        const int* gnb[32];         /* per (slot k, other slot): its vertex per incident edge */ \
        int nedge[4];               /* edges per graph */                                   \
        unsigned char* flags;       /* bit0: active (not excluded) */                       \
        long long uoff[4];          /* offset of each unknown image in the vector */        \
        int ymem0;                  /* 2-D row slabs: global row of memory row 0 */          \
        long long own_lo, own_hi;   /* owned pixels (memory indices) */
#define OPTAMD_GENARGS_LOSS                                                                 \
        void* lwe[4];               /* per loss group: its edges' weights (T), edge order */ \
        void* lwq[16];              /* per (group, slot) of GenSource::loss_inc: the same weights in that slot's incidence order */ \
        const int* lpos[16];        /* per slot: position of each edge in the slot's incidence list */
#define OPTAMD_GENARGS_SPACES                                                               \
        int sdims[8][3];            /* per space: its dims, unused dims = 1 */               \
        long long snpix[8];         /* per space: its elements */                            \
        long long fbase[8];         /* per unknown-carrying space: first flag byte */

namespace optamd {
struct GenArgs {
    OPTAMD_GENARGS_FIELDS
    OPTAMD_GENARGS_SPACES
    OPTAMD_GENARGS_LOSS
};
namespace gen {

// explicit Schur complement: a block of S with more pairs than this is assembled by a whole
// workgroup (gen_schur_assemble_long; the host lists such blocks), the others by one wave each
constexpr int kSchurLongPairs = 128;
// explicit J^T J: gen_normal_spmv gives a block row to C lanes of a wave, which walk it block
// after block; a row with more blocks than this (a hub vertex; the host lists such rows) is
// summed by a whole workgroup instead, the form of gen_schur_spmv. That form pays two barriers
// and 256 / C values added from LDS by C lanes per row, about what 64 more blocks cost the
// lane group, whose wave meanwhile waits for its longest row (reasoned, not measured).
constexpr int kNormalLongRow = 64;

struct GenSource {
    std::string code;
    bool has_centered = false;   // centred residuals present
    bool has_graph = false;      // graph residuals present
    int slot_base[4] = {0, 0, 0, 0};   // GenArgs::slot index of graph g's first vertex array
    int n_precompute = 0;              // kernels gen_precompute_0 .. n-1 (ComputedArrays)
    bool has_tiled = false;            // gen_apply_tiled emitted (2-D centred energies)
    int tiles_x = 32, tiles_y = 8;     // its output tile
    size_t tiled_lds = 0;              // its LDS bytes
    double instances_per_residual = 0; // distinct (residual, shift) instances / centred residuals
    bool prefer_tiled = false;         // the plan's default apply (static rule, codegen.cpp)
    bool has_strip = false;            // gen_apply_strip emitted (2-D centred, no sampled reads)
    int strip_cols = 64;               // its output columns per wave
    bool has_jtf_strip = false;        // gen_jtf_strip emitted (the same walk for J^T F)
    int jtf_strip_cols = 64;
    bool has_cost_strip = false;       // gen_cost_strip emitted (centred-only 2-D energies)
    int cost_strip_cols = 64;
    // materialized J (saveJToCRS): one kernel gen_dump_j_<i> per energy spec, in order;
    // spec i: domain (-1 centred, else graph id), residual rows and nonzeros per element
    struct DumpSpec { int graph; int rows; int nnz; };
    std::vector<DumpSpec> dump;
    // GenArgs::gnb[i] = slot nb_pairs[i].second's vertex of each edge in slot
    // nb_pairs[i].first's incidence order (the graph gathers read neighbours through it)
    std::vector<std::pair<int, int>> nb_pairs;
    // gen_apply_graph adds the centred residuals' terms itself (1-D vertex domains): the
    // plan launches no gen_apply before it
    bool graph_apply_centred = false;
    // gen_schur_rhs / gen_schur_elim / gen_schur_apply emitted (Eliminate, codegen_schur.cpp)
    bool has_schur = false;
    // ReducedSystem("explicit") (codegen_schur_explicit.cpp): gen_schur_eblk, gen_schur_assemble
    // and gen_schur_spmv emitted. Cr / Ce: channels of the retained / eliminated group, the
    // retained group's space. Each list is one (eliminated slot, retained slot) pair of one
    // graph, as GenArgs::slot indices: its instances are the edges in the eliminated slot's
    // incidence order, and instance q of list l sits at position (sum of the earlier lists'
    // edge counts) + q of the per-instance buffers.
    bool has_schur_explicit = false;
    int schur_cr = 0, schur_ce = 0, schur_rspace = -1;
    struct SchurList { int graph; int eslot; int rslot; };
    std::vector<SchurList> schur_lists;
    // NormalMatrix("explicit") (codegen_normal.cpp): gen_normal_eblk, gen_normal_assemble and
    // gen_normal_spmv emitted. C: channels of the one block group, R: residuals per edge (the
    // largest graph's; G_q is C x R), the group's space. Each list is one slot over that space
    // of one graph (a GenArgs::slot index); instance e of list l, edge e seen from that slot,
    // sits at position (sum of the earlier lists' edge counts) + e.
    bool has_normal = false;
    int normal_c = 0, normal_r = 0, normal_space = -1;
    struct NormalList { int graph; int slot; };
    std::vector<NormalList> normal_lists;
    // LinearSolver("cholesky") beside one of the two explicit forms (codegen_dense.cpp):
    // gen_dense_fill and gen_dense_store emitted
    bool has_dense = false;
    // RobustEnergy (GModel::loss): gen_loss_weights emitted. loss_inc[i] = (group, GenArgs::slot
    // index): GenArgs::lwq[i] holds that group's weights in that slot's incidence order — one
    // entry per slot through which the group's residuals read an unknown
    bool has_loss = false;
    std::vector<std::pair<int, int>> loss_inc;
};

// Generate the kernels for `m` in float (dbl = false) or double. off32: every array a
// graph gather reads (the unknown vectors, known and internal images, the incidence
// copies) is below 2 GiB, so slot reads address it as a uniform base plus a 32-bit byte
// offset (the plan checks the sizes).
GenSource generate(GModel& m, bool dbl, bool off32 = false);

}  // namespace gen
}  // namespace optamd
