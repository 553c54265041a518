/*
 * opt_amd.h — extension entry points of libopt_amd.so beyond the reference ABI.
 *
 * The reference exposes its solver only through Opt.h; its kernels are reachable
 * only from inside the generated step() (solverGPUGaussNewton.t:1913-2349). These
 * entry points expose the same kernels one at a time so the parity tests and the
 * benchmark can drive and time them without a full solve. Each cites the reference
 * kernel whose per-unknown result it returns. All pointers are device pointers into
 * the plan's unknown-vector layout: one contiguous block per unknown image in
 * declaration order, channels interleaved inside an image (reference UnknownType,
 * API/src/o.t:998-1100; e.g. image_warping = [Offset.xy * N | Angle * N]).
 * Element type is float, or double when the state was created with doublePrecision.
 * All calls are synchronous (they return after the device work completed).
 * Return value 0 = success, nonzero = invalid arguments (message on stderr).
 */
#pragma once
#include "Opt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Total number of scalar unknowns of the plan (e.g. 3*W*H for image_warping). */
long long OptAMD_PlanUnknownCount(Opt_Plan* plan);

/* The unknown vector r, pre, p and Ap are laid out over: one contiguous block per unknown
 * image, in problemparams order, channels interleaved. For each of the first maxImages
 * images writes the block's first element, its element (pixel) count and its channels
 * (any of the three arrays may be NULL); the blocks differ in length when the unknowns
 * lie over several index spaces. Returns the number of unknown images, -1 on a null plan. */
int OptAMD_PlanUnknownLayout(Opt_Plan* plan, int maxImages, long long* offset, long long* elements,
                             int* channels);

/* Energy family the problem was lowered to ("image_warping", "poisson_image_editing",
 * ...); writes a NUL-terminated name into buf. Returns the name length. */
int OptAMD_PlanFamily(Opt_Plan* plan, char* buf, int buflen);

/* Kernel family Opt_ProblemDefine chose for the energy file: a hand-written family
 * only when the file lowers to exactly that family's residual templates, else
 * "generic" (kernels generated from the file at plan time). No device needed. */
int OptAMD_ProblemFamily(Opt_Problem* problem, char* buf, int buflen);

/* Structural signature of an energy file as the front end lowers it (declaration
 * kinds/types/indices, ComputedArray, Exclude and residual templates; names dropped):
 * two files with equal signatures define the same problem. Returns the length, or -1
 * with the error message in buf. No device needed. */
int OptAMD_GenericSignature(const char* filename, char* buf, int buflen);

/* r = -J^T F and the CERES-guarded Jacobi preconditioner pre = 1/(1+sqrt(diag J^TJ))^2
 * (or the reference's forced value when UsePreconditioner(false)) at the current
 * unknowns; *r_dot_pre_r = sum r.(pre*r) (reference kernels.PCGInit1,
 * solverGPUGaussNewton.t:521-563, with fmap.evalJTF o.t:2870-2913). Excluded
 * elements get r = 0, pre = 0. On a plan with the block preconditioner (below) pre is
 * still this scalar preconditioner: the blocks are applied by OptAMD_ApplyPreconditioner. */
int OptAMD_EvalJTF(Opt_State* state, Opt_Plan* plan, void** problemparams,
                   void* r, void* pre, double* r_dot_pre_r);

/* Block-Jacobi preconditioner: UsePreconditioner("block") in an energy file (the reference
 * reads any non-nil argument as true, so the file runs there with the scalar
 * preconditioner). A block group is one index space that holds unknowns: its unknown
 * images in problemparams order, C = the sum of their channels (at most 8, else
 * Opt_ProblemDefine returns NULL). For element e, B_e is the C x C diagonal block of J^T J
 * over that element's channels; PCG is preconditioned with M_e^-1, M_e = B_e on a
 * gaussNewtonGPU plan and B_e + diag(CtC_e) (the clamped LM diagonal) on an LMGPU plan.
 * M_e is factored by Cholesky; where a pivot is <= eps * C * max_i (M_e)_ii (eps: the
 * machine epsilon of the solver precision) the element uses the diagonal matrix of the
 * scalar preconditioner's values instead. Excluded elements get M_e^-1 = 0. Such energies
 * run on generated kernels only and refuse OptAMD_PlanSetDecomposition.
 *
 * Writes, for each unknown image (OptAMD_PlanUnknownLayout order, up to maxImages), its
 * block group and the row of its first channel inside the block; returns the number of
 * groups, 0 for a plan with the scalar preconditioner, -1 for a NULL plan. */
int OptAMD_PlanPreconditionerBlocks(Opt_Plan* plan, int maxImages, int* group, int* firstRow);

/* z = M^-1 r for the caller's r (device vectors of OptAMD_PlanUnknownCount elements) with
 * the preconditioner evaluated at the current unknowns: the GN form on a gaussNewtonGPU
 * plan, the LM form with the plan's current trust-region radius on an LMGPU plan. On a
 * plan with the scalar preconditioner z = pre * r. Returns 0, or 1 where the plan has no
 * such entry point (the hand-written image_warping plan). */
int OptAMD_ApplyPreconditioner(Opt_State* state, Opt_Plan* plan, void** problemparams,
                               const void* r, void* z);

/* Schur complement: Eliminate(X, ...) in an energy file names the unknown images of one
 * index space (all of them, and another unknown-carrying space must remain), whose block C
 * of A = J^T J (+ LM's diagonal) = [[B, E], [E^T, C]] is block-diagonal: one block per
 * element, no residual reads two elements of the group (else Opt_ProblemDefine returns
 * NULL and names the cause). The statement turns the block preconditioner on. PCG then runs
 * on S delta_r = b_r - E M^-1 b_e, S = B - E M^-1 E^T, preconditioned with the retained
 * groups' blocks, and delta_e = M^-1 (b_e - E^T delta_r) follows; M_e = C_e, or
 * C_e + diag(CtC_e) on an LMGPU plan. An eliminated element whose Cholesky pivot is
 * <= sqrt(eps) * max_i (M_e)_ii is held fixed for that step (M_e^-1 = 0), as excluded
 * elements are. The unknown vector keeps its layout (OptAMD_PlanUnknownLayout).
 *
 * Writes, for each unknown image (layout order, up to maxImages), 1 if the plan eliminates
 * it, else 0 (all 0 on a plan without the statement); returns the number of unknown images,
 * -1 for a NULL plan. */
int OptAMD_PlanEliminated(Opt_Plan* plan, int maxImages, int* eliminated);

/* Robust losses: RobustEnergy(kind, scale, term, ...) in the energy file (generated kernels;
 * INTEGRATION.md, "Robust losses"). The statement's scalar residuals f_1..f_R form one loss
 * block per edge of their graph, s = sum f_k^2; kind "huber" (rho = s up to a^2, then
 * 2 a sqrt(s) - a^2) or "cauchy" (rho = a^2 log(1 + s / a^2)); the scale a is a positive number
 * or a float Param, re-read whenever the weights are evaluated. The cost is 1/2 sum rho(s) plus
 * the plain terms; each linearisation is that of the reweighted problem f~ = w f, J~ = w J with
 * w = sqrt(rho'(s)) held constant (IRLS, no second-order correction), one cached weight per
 * edge. At most 4 statements per file.
 *
 * Writes, for each loss group (statement order, up to maxGroups), its graph, its residuals per
 * edge and its kind (0 huber, 1 cauchy); any array may be NULL. Returns the number of groups:
 * 0 on a plan without the statement, -1 for a NULL plan. */
int OptAMD_PlanLossGroups(Opt_Plan* plan, int maxGroups, int* graph, int* residuals, int* kind);

/* Edges of loss group `group`'s graph (the length of OptAMD_EvalLossWeights' array); -1 for a
 * NULL plan or a group the plan does not have. */
long long OptAMD_PlanLossGroupEdges(Opt_Plan* plan, int group);

/* rho'(s) of every edge of loss group `group` at the bound unknowns, in edge order, into
 * `weights`: an array of the plan's precision with the graph's edge count (a device array;
 * a host array on a backend_cpu state). Note rho', not its root: 1 on an inlier of the Huber
 * loss, below 1 where the loss bends. Returns 0; 1 on a plan without the statement; 1 with
 * OptAMD_PlanError set for a group out of range. */
int OptAMD_EvalLossWeights(Opt_State* state, Opt_Plan* plan, void** problemparams, int group, void* weights);

/* Sp = S p at the current unknowns (device vectors of OptAMD_PlanUnknownCount elements;
 * on an LMGPU plan with CtC_r p and M at the plan's current trust-region radius). The
 * eliminated entries of p are ignored, those of Sp are 0. Returns 0, or 1 on a plan without
 * Eliminate. OptAMD_ApplyJTJ on such a plan is still the full J^T J p. */
int OptAMD_ApplyReduced(Opt_State* state, Opt_Plan* plan, void** problemparams,
                        const void* p, void* Sp);

/* The explicitly formed reduced system: ReducedSystem("explicit") beside Eliminate makes the
 * plan assemble S once per Step in block-CSR (blocks of blockDim x blockDim, blockDim the
 * retained element's channel count, row-major inside a block; rows and columns are retained
 * elements, columns ascending, every diagonal block present) and run PCG's apply as a block
 * SpMV. LM's retained diagonal is not part of S (the apply adds it). The pattern follows the
 * graphs' vertex arrays as bound and is rebuilt when they are re-wired between Steps.
 * ReducedSystem("implicit"), or no statement, is the matrix-free apply. Shapes the explicit
 * form does not take are refused by Opt_ProblemPlan by name.
 *
 * Returns 1 and the shape on an explicit plan once the graphs have been bound (by Init, Step,
 * or any entry point that takes problemparams), 0 on any other plan or before, -1 for NULL. */
int OptAMD_PlanReducedMatrixShape(Opt_Plan* plan, long long* blockRows, int* blockDim, long long* nnzBlocks);

/* S assembled at the bound unknowns (on an LMGPU plan with M at the plan's current
 * trust-region radius), copied into caller device arrays: rowPtr blockRows + 1, colInd
 * nnzBlocks, val nnzBlocks * blockDim^2 in the plan's precision. With all three NULL the call
 * binds the arrays and builds the pattern only, so that OptAMD_PlanReducedMatrixShape can size
 * them. Returns 0, or 1 on a plan without an explicit reduced system. */
int OptAMD_ReducedMatrix(Opt_Plan* plan, void** problemparams, int* rowPtr, int* colInd, void* val);

/* The symbolic phase behind that pattern, on the host from index arrays alone (no device):
 * list l has nEdges[l] edge instances with eliminated vertex elimVertex[l][e] and retained
 * vertex retVertex[l][e]. Instance positions: list after list, each list ordered by eliminated
 * vertex, ties by edge index. Every output may be NULL; counts receives {instances, pairs,
 * blocks}; pairPtr has blocks + 1 entries and pairs two positions (q1, q2) per pair. Returns 0,
 * or -1 with the cause in buf (an index outside its space, more than 2^31 - 1 pairs). */
int OptAMD_SchurPattern(long long nEliminated, long long nRetained, int nLists, const int* const* elimVertex,
                        const int* const* retVertex, const long long* nEdges, long long* counts, int* rowPtr,
                        int* colInd, int* pairPtr, int* pairs, char* buf, int buflen);

/* The same symbolic phase run by the device builder a plan uses (sorts and scans on the current
 * device's null stream): host arrays in, host arrays out, the index check on the host as above,
 * every array equal to OptAMD_SchurPattern's element for element, the refusals word for word.
 * Needs a device but no plan and no energy file. */
int OptAMD_SchurPatternDevice(long long nEliminated, long long nRetained, int nLists, const int* const* elimVertex,
                              const int* const* retVertex, const long long* nEdges, long long* counts, int* rowPtr,
                              int* colInd, int* pairPtr, int* pairs, char* buf, int buflen);

/* Where the last symbolic phase of an explicit S or H ran, one line of key=value words in buf:
 *   path=device|host reason=default|env|memory pairs=N blocks=N instances=N transient_bytes=N
 * A plan builds the pattern on the device; OPT_AMD_SYMBOLIC=host|device, read when the plan is
 * made, selects the path (reason=env). A wiring whose device temporaries (transient_bytes)
 * exceed the free device memory less the buffers that stay, or OPT_AMD_SYMBOLIC_MAX_BYTES when
 * set, takes the host path without an error (path=host reason=memory). Returns the line's
 * length (0, an empty line, before the first symbolic phase), -1 on a plan with neither
 * ReducedSystem("explicit") nor NormalMatrix("explicit"), or for NULL. */
int OptAMD_PlanSymbolicInfo(Opt_Plan* plan, char* buf, int buflen);

/* The direct solver: LinearSolver("cholesky") in an energy file beside ReducedSystem("explicit")
 * or NormalMatrix("explicit") makes every Step with lIterations > 0 take the exact Gauss-Newton /
 * LM step: the assembled S or H plus LM's clamped diagonal is filled into 64 x 64 tiles of a
 * dense lower triangle (rows and columns of excluded elements as identity rows), factored
 * A = L L^T by the blocked MFMA kernels of OptAMD_DenseCholesky and solved for the retained
 * delta; back-substitution, update, model cost and LM's accept / revert follow as after PCG.
 * lIterations only switches the linear solve on (> 0) or off; q_tolerance and
 * residual_reset_period do not apply. LinearSolver("pcg"), or no statement, is the PCG loop.
 * A Step falls back to the explicit plan's PCG loop, bitwise what the file without the statement
 * does, when the dense storage exceeds OPT_AMD_DENSE_MAX_BYTES (default 2 GiB) or the free
 * device memory (reason=memory), or when a pivot fails: NaN, not positive, or <= eps * the row's
 * original diagonal entry (reason=pivot; the host reads the flag once per Step after the
 * factorisation). One line of key=value words in buf:
 *   n=N tiles=N bytes=N factorisations=N fallbacks=N reason=none|memory|pivot min_pivot_ratio=X
 *   covariances=N cov_bytes=N                                   (OptAMD_Covariance, below)
 * n the padded-free dimension, tiles the stored 64 x 64 tiles, bytes the dense storage,
 * factorisations / fallbacks the Steps that took either path, reason the last fall-back's,
 * min_pivot_ratio the smallest pivot / original diagonal of the last completed factorisation (inf before
 * the first). Returns the line's length, -1 on a plan without the statement, or for NULL. */
int OptAMD_PlanDirectInfo(Opt_Plan* plan, char* buf, int buflen);

/* The explicitly formed normal matrix: NormalMatrix("explicit") in an energy file whose unknowns
 * lie over one index space makes the plan assemble H = J^T J once per Step in block-CSR (blocks
 * of blockDim x blockDim, blockDim the channels of all unknowns of one element, row-major inside
 * a block; rows and columns are elements, columns ascending, every diagonal block present) and
 * run every apply of PCG, and OptAMD_ApplyJTJ, as a block SpMV. The statement turns the block
 * preconditioner on, as UsePreconditioner("block") does. LM's diagonal is not part of H (the
 * apply adds it); excluded elements keep their rows and columns in H (the apply masks the rows).
 * The pattern follows the graphs' vertex arrays as bound and is rebuilt when they are re-wired
 * between Steps. NormalMatrix("matrix_free"), or no statement, is the gather apply. Shapes the
 * explicit form does not take are refused by Opt_ProblemPlan by name, as are
 * useMaterializedJTJ / useFusedJTJ on such a plan; a file with Eliminate uses ReducedSystem.
 *
 * Returns 1 and the shape on such a plan once the graphs have been bound (by Init, Step, or any
 * entry point that takes problemparams), 0 on any other plan or before, -1 for NULL. */
int OptAMD_PlanNormalMatrixShape(Opt_Plan* plan, long long* blockRows, int* blockDim, long long* nnzBlocks);

/* H assembled at the bound unknowns, copied into caller device arrays: rowPtr blockRows + 1,
 * colInd nnzBlocks, val nnzBlocks * blockDim^2 in the plan's precision. With all three NULL the
 * call binds the arrays and builds the pattern only, so that OptAMD_PlanNormalMatrixShape can
 * size them. Returns 0, or 1 on a plan without an explicit normal matrix. */
int OptAMD_NormalMatrix(Opt_Plan* plan, void** problemparams, int* rowPtr, int* colInd, void* val);

/* The symbolic phase behind that pattern, on the host from index arrays alone (no device): graph
 * g has graphEdges[g] edges; list l is one slot of graph listGraph[l] over the unknowns' space,
 * vertex[l][e] its vertex at edge e. Instance positions: list after list, edge e of a list at
 * its base + e. For every edge, every ordered pair of two different instances (q1, q2), in the
 * order [list, edge], goes to block (vertex(q1), vertex(q2)). Every output may be NULL; counts
 * receives {instances, pairs, blocks}; pairPtr has blocks + 1 entries and pairs two positions
 * per pair. Returns 0, or -1 with the cause in buf. */
int OptAMD_NormalPattern(long long nVertices, int nLists, const int* const* vertex, const int* listGraph,
                         const long long* graphEdges, int nGraphs, long long* counts, int* rowPtr, int* colInd,
                         int* pairPtr, int* pairs, char* buf, int buflen);

/* The same on the device, as OptAMD_SchurPatternDevice is to OptAMD_SchurPattern. */
int OptAMD_NormalPatternDevice(long long nVertices, int nLists, const int* const* vertex, const int* listGraph,
                               const long long* graphEdges, int nGraphs, long long* counts, int* rowPtr, int* colInd,
                               int* pairPtr, int* pairs, char* buf, int buflen);

/* A dense Cholesky factorisation and solve on the current device, with no plan and no energy
 * file: A (n x n, row-major, symmetric positive definite; both triangles are read) and b are
 * host arrays of float, or of double with isDouble != 0. The matrix is packed into 64 x 64 tiles
 * of the lower triangle (n padded to a multiple of 64 with an identity), factored A = L L^T by
 * the blocked right-looking MFMA kernels and solved by the two triangular launch chains; L_out
 * (n x n, row-major, lower triangle, zeros above) and x_out (n) receive the factor and the
 * solution of A x = b. *info is -1, or the first row whose pivot failed: NaN, not positive, or
 * <= eps * a_ii of the precision; then every later kernel of the chain returns at entry and
 * L_out and x_out are left untouched. Two calls on the same inputs agree bitwise. Returns 0,
 * or -1 for invalid arguments or a matrix whose storage does not fit the device. */
int OptAMD_DenseCholesky(long long n, const void* A, const void* b, void* L_out, void* x_out, int isDouble,
                         long long* info);

/* Marginal covariances: selected blockDim x blockDim blocks of A^-1, A the plan's assembled S or
 * H at the bound unknowns WITHOUT LM's diagonal (on an LM plan with Eliminate the eliminated
 * blocks are inverted undamped too), from the dense Cholesky factor of LinearSolver("cholesky").
 * The call binds the arrays, assembles the matrix as OptAMD_NormalMatrix / OptAMD_ReducedMatrix
 * do (robust terms with their weights), fills and factors the tiles the direct Step uses, and
 * forms Y = L^-1 E for the identity columns E of the selected unknowns by a forward launch chain
 * of MFMA tile products, then block (s, t) = Y_s^T Y_t. Work and storage follow the selection:
 * tiles of Y left of an element's first unknown are never formed. rowElem / colElem are host
 * arrays of nPairs element numbers, numbered as the block rows of OptAMD_PlanNormalMatrixShape /
 * OptAMD_PlanReducedMatrixShape; blocks is a device array blocks[nPairs][blockDim][blockDim] in
 * the plan's precision. Blocks of an excluded or held element, and its cross blocks, are zeros.
 * The call leaves the unknowns, the cost, the LM state and the next Step (bitwise) as they were.
 * Returns 0; -1 for NULL or an element out of range; 1 on a plan without LinearSolver("cholesky");
 * 2 when the tiles plus the selection's workspace exceed OPT_AMD_DENSE_MAX_BYTES (read at each
 * call) or the free device memory (reason=memory: no fall-back, no chunking); 3 when a pivot
 * fails (reason=pivot: gauge freedom; blocks untouched). OptAMD_PlanError holds the message, for
 * a pivot with the row, the element and the channel. OptAMD_PlanDirectInfo's line ends in
 * covariances=N cov_bytes=N: the calls completed and the last workspace. */
int OptAMD_Covariance(Opt_State* state, Opt_Plan* plan, void** problemparams, long long nPairs, const int* rowElem,
                      const int* colElem, void* blocks);

/* The same kernels with no plan: blocks of A^-1 for a host matrix A (n x n, row-major, symmetric
 * positive definite; float, or double with isDouble != 0) cut into elements of C unknowns (n a
 * multiple of C, 1 <= C <= 64). rowElem / colElem and out[nPairs][C][C] are host arrays. *info is
 * -1, the first row whose pivot failed (out untouched), or -2 when the storage does not fit the
 * device. Returns 0, or -1 for invalid arguments (an element out of range among them), before
 * any launch. */
int OptAMD_DenseInverseBlocks(long long n, const void* A, int C, long long nPairs, const int* rowElem, const int* colElem,
                              void* out, int isDouble, long long* info);

/* Ap = J^T J p at the current unknowns (+ CtC*p for LM plans, with the CtC of the
 * last LM step) and *p_dot_Ap = p.Ap (reference kernels.PCGStep1,
 * solverGPUGaussNewton.t:607-632, with fmap.applyJTJ o.t:2770-2830). Excluded
 * elements get Ap = 0. */
int OptAMD_ApplyJTJ(Opt_State* state, Opt_Plan* plan, void** problemparams,
                    const void* p, void* Ap, double* p_dot_Ap);

/* Energy 1/2 sum r^2 at the current unknowns (reference kernels.computeCost,
 * solverGPUGaussNewton.t:971-997, fmap.cost o.t:3119-3129). */
double OptAMD_EvalCost(Opt_State* state, Opt_Plan* plan, void** problemparams);

/* Launch the apply `reps` times back to back on the plan's stream, bracketed by
 * hipEvents; returns the mean device time per launch in microseconds. */
double OptAMD_TimeApplyJTJ(Opt_State* state, Opt_Plan* plan, void** problemparams,
                           const void* p, void* Ap, int reps);

/* Per-kernel device-time accounting (hipEvent pairs on the plan's stream).
 * mode 0: off; 1: every kernel (the reference's collectPerKernelTimingInfo);
 * 2: only the PCG J^T J p apply kernel. Resets the accumulated statistics. */
void OptAMD_SetKernelTiming(Opt_Plan* plan, int mode);

/* Accumulated statistics for kernel `name` since the last reset: number of launches
 * and total device milliseconds. Returns 0 if the kernel was seen, 1 otherwise. */
int OptAMD_KernelStat(Opt_Plan* plan, const char* name, long long* launches, double* total_ms);

/* Name of the plan's dominant (PCG apply) kernel as it appears in KernelStat and in
 * rocprofv3 kernel traces. */
int OptAMD_ApplyKernelName(Opt_Plan* plan, char* buf, int buflen);

/* Which forms of the generated kernels this plan launches, after the OPT_AMD_GEN_APPLY / _JTF /
 * _COST knobs, the wave-count rule, row slabs and the block preconditioner, as one line of
 * key=value words: "apply=gather|tiled|strip jtf=gather|strip cost=gather|strip grid=<blocks>
 * rows=<image rows> apply_row_block=<rows> jtf_row_block=<rows> cost_row_block=<rows>
 * materialized=0|1" (a strip form walks blocks of that many rows per wave; 0 for the other
 * forms). Returns the length, or -1 on a plan that is not on generated kernels. */
int OptAMD_PlanGeneratedForms(Opt_Plan* plan, char* buf, int buflen);

/* Human-readable table of every timed kernel (reference timer report,
 * backend_cuda.t:231-297). Returns the length written. */
int OptAMD_KernelReport(Opt_Plan* plan, char* buf, int buflen);

/* The HIP stream (hipStream_t) all of the plan's device work is issued on. */
void* OptAMD_PlanStream(Opt_Plan* plan);

/* Outer iterations completed since the last Init. */
int OptAMD_PlanIterations(Opt_Plan* plan);

/* Copy up to n of the plan's device scalar slots (fp64: costs, the PCG rz / pAp sums of
 * the last Step, ...) to `out` after synchronising; returns the number copied. The slot
 * layout is the family's (image_warping: opt_amd/csrc/image_warping.hip, kScBase /
 * kSlots); a parity/diagnostic hook with no reference counterpart. */
int OptAMD_PlanScalars(Opt_Plan* plan, double* out, int n);

/* ---- multi-GPU row-slab decomposition (no reference counterpart:
 * the reference is single-device, §2.3) ------------------------------------------ */
typedef struct OptAMD_Comm OptAMD_Comm;
typedef struct OptAMD_LocalGroup OptAMD_LocalGroup;

/* 128-byte RCCL unique id, created on one rank and shared with the others by the
 * caller (e.g. torch.distributed broadcast). Returns 0 on success. */
int OptAMD_RcclUniqueId(void* out128);
/* RCCL communicator over `nranks` processes, one GPU each (the current HIP device). */
OptAMD_Comm* OptAMD_CommCreateRccl(const void* id128, int rank, int nranks);
void OptAMD_CommDestroy(OptAMD_Comm* comm);
/* Number of ranks / this rank of a communicator (-1 for NULL): bench.py reports the
 * world size the solver actually runs on from here, not from the launcher's env. */
int OptAMD_CommSize(OptAMD_Comm* comm);
int OptAMD_CommRank(OptAMD_Comm* comm);
/* The transport behind a communicator, "rccl" or "local", copied into buf (at most
 * buflen bytes incl. the terminator); returns its length, -1 for NULL. */
int OptAMD_CommKind(OptAMD_Comm* comm, char* buf, int buflen);
/* The error that stopped the last Init / Step of this plan (a problem found only when
 * the arrays were bound, e.g. an arap graph whose adjacency exceeds 2^31 slots), copied
 * into buf; returns its length, 0 when there was none (-1 for NULL). After such an
 * error Opt_ProblemStep returns 0 and Opt_ProblemCurrentCost NaN; the process goes on.
 * Where there is none, the refusal of the last OptAMD_Covariance (reason=memory, reason=pivot, a
 * bad index, no statement), which stops nothing and which the next Init or Step clears. */
int OptAMD_PlanError(Opt_Plan* plan, char* buf, int buflen);
/* All ranks as threads of one process (shared device or peer devices): for testing
 * the decomposition on one GPU. The rank handles belong to the group. */
OptAMD_LocalGroup* OptAMD_LocalGroupCreate(int nranks);
OptAMD_Comm* OptAMD_LocalGroupRank(OptAMD_LocalGroup* group, int rank);
void OptAMD_LocalGroupDestroy(OptAMD_LocalGroup* group);

/* Stencil radius of the plan's energy (rows of neighbour data a slab needs). */
int OptAMD_PlanHalo(Opt_Plan* plan);
/* Make this plan one rank of a row-slab decomposition of the dims given to
 * Opt_ProblemPlan: it owns global rows [y_lo, y_hi). From then on every array in
 * problemparams (and every vector passed to the OptAMD_ kernels) holds rows
 * [y_lo - hl, y_hi + hh) with hl = min(halo, y_lo), hh = min(halo, H - y_hi); the
 * caller fills the known arrays' halo rows, the plan refreshes the unknowns' halo rows
 * itself. Energies, costs and dot products are global (summed over ranks).
 * Returns 0 on success. */
int OptAMD_PlanSetDecomposition(Opt_Plan* plan, OptAMD_Comm* comm, int y_lo, int y_hi);

/* ---- materialized Jacobian path (useMaterializedJTJ / useFusedJTJ, Opt.h) --------
 * Every array is a device pointer; CSR is zero-based with int32 indices (nnz < 2^31);
 * values are float, or double when doublePrecision is nonzero. Synchronous. */

/* Shape of the plan's assembled Jacobian: returns its nonzero count and stores the
 * residual (row) count in *nResiduals; -1 when the energy family has no J assembly. */
long long OptAMD_PlanJacobianShape(Opt_Plan* plan, long long* nResiduals);

/* Nonzeros of the J and (fused) J^T J a materialized plan holds (the J^T J count is
 * known after the first Step, 0 before and for useFusedJTJ = 0). Returns 1 for a
 * matrix-free plan. */
int OptAMD_PlanMaterializedNonzeros(Opt_Plan* plan, long long* nnzJ, long long* nnzJTJ);

/* J at the current unknowns (reference kernels.saveJToCRS, solverGPUGaussNewton.t:
 * 1004-1022, rows/columns as generateDumpJ :385-442: one block of rows per pixel,
 * columns = unknown indices wrapped into [0, nUnknowns) and sorted inside each row).
 * rowPtr: nResiduals+1, colInd / val: nnz. Returns 0 on success. */
int OptAMD_EvalJacobian(Opt_State* state, Opt_Plan* plan, void** problemparams,
                        int* rowPtr, int* colInd, void* val);

/* A^T of an nRowsA x nColsA matrix: rowPtrAT (nColsA+1), colIndAT and valAT (nnz), the
 * rows of A ascending inside each row of A^T (reference computeNnzPatternAT + computeAT,
 * API/src/linalg_cpu.t:203-297,512-551; cusparseScsr2csc, API/src/backend_cuda.t:600-612).
 * valA / valAT may be NULL (pattern only). The column indices of every row of A must be
 * strictly ascending (no repeated column inside a row), the reference's contract for its
 * CSR matrices: computeAT reads A(row, col) with getEntry, which takes the first match. */
int OptAMD_CsrTranspose(int nRowsA, int nColsA, long long nnz, const int* rowPtrA,
                        const int* colIndA, const void* valA, int* rowPtrAT, int* colIndAT,
                        void* valAT, int doublePrecision);

/* A^T A (nColsA x nColsA) of A. The column indices of every row of A must be strictly
 * ascending: sorted, and no column repeated inside a row. This is the reference's
 * contract (computeATA walks each row of A once against the sorted A^T A row, so a
 * repeated or out-of-order column, and every entry of the row after it, is dropped from
 * the sums); nothing checks it. First call with
 * colIndATA = valATA = NULL: fills rowPtrATA (nColsA+1) and *nnzATA; second call with
 * those arrays allocated: sorted column indices and the values, each summed over the
 * rows of A in ascending order (reference computeNnzPatternATA + computeATA,
 * API/src/linalg_cpu.t:300-508; cusparseXcsrgemmNnz / cusparseScsrgemm,
 * API/src/backend_cuda.t:556-596). Nonzero return: more than 2^31 nonzeros. */
int OptAMD_CsrATA(int nRowsA, int nColsA, long long nnz, const int* rowPtrA, const int* colIndA,
                  const void* valA, int* rowPtrATA, int* colIndATA, void* valATA,
                  long long* nnzATA, int doublePrecision);

/* y = A x (reference applyAtoVector, API/src/linalg_cpu.t:560-600; cusparseScsrmv,
 * API/src/backend_cuda.t:616-636). */
int OptAMD_CsrSpMV(int nRowsA, int nColsA, long long nnz, const int* rowPtrA, const int* colIndA,
                   const void* valA, const void* x, void* y, int doublePrecision);

/* General energy front end (the reference's energy compiler, API/src/o.t:1295-1348 and
 * 2669-3235): the HIP source generated for the energy file `filename` (float kernels, or
 * double with bit 0 of doublePrecision set; bit 1 selects the 32-bit gather addressing a
 * plan takes when its arrays are below 2 GiB), copied into buf (NUL-terminated, truncated
 * to n). Returns the full length, or -1 with the front end's message in buf. No device
 * needed. */
int OptAMD_GenericSource(const char* filename, int doublePrecision, char* buf, int n);

/* The checks Opt_ProblemPlan makes on the lowered energy before it asks for a device (the
 * shapes ReducedSystem("explicit") takes). 0 accepted, 1 refused with the plan's message in
 * buf, -1 with the front end's message if the file does not lower. No device needed. */
int OptAMD_GenericPlanCheck(const char* filename, char* buf, int n);

/* The residual templates the front end lowered `filename` to, one line each:
 * "<centred|graphK> <number of unknowns it reads> <expression>" (the reference's
 * toenergyspecs / classifyexpression result, API/src/o.t:2669-2715). Returns the residual
 * count, or -1 with the front end's message in buf. */
int OptAMD_GenericDescribe(const char* filename, char* buf, int n);

/* What the generator emitted for `filename` beside the gathers, as one line of key=value
 * words: "has_tiled tiles_x tiles_y has_strip strip_cols has_jtf_strip jtf_strip_cols
 * has_cost_strip cost_strip_cols" (a form that cannot serve the energy, or whose row windows
 * pass the register cap, is not emitted, and a plan then keeps the gather). Returns the
 * length, or -1 with the front end's message in buf. No device needed. */
int OptAMD_GenericForms(const char* filename, int doublePrecision, char* buf, int n);

/* Compile that source for gfx950 with hiprtc (no device needed). 0 on success, -1 with
 * the compiler log (or the front end's message) in buf. */
int OptAMD_GenericCompileCheck(const char* filename, int doublePrecision, char* buf, int n);

#ifdef __cplusplus
}
#endif
