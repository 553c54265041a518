"""ctypes binding of libopt_amd.so and a Python mirror of the reference's OptSolver.

Mirrors examples/shared/OptSolver.h:46-106 (state/problem/plan lifetime, solve) and
examples/shared/OptUtils.h:47-64 (profiled Init/Step loop) and 108-112 (solver
parameters by name). Problem parameters are passed exactly as the reference's
NamedParameters::data() packs them (examples/shared/NamedParameters.h:35-49): one
``void*`` per declared index — a device (or, for the CPU backends, host) array
pointer for Array/Unknown, a pointer to the value for Param.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, List, Optional, Sequence

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libopt_amd.so")


class OptError(RuntimeError):
    pass


class InitParams(ctypes.Structure):
    """Opt_InitializationParameters (include/Opt.h; reference Opt.h:10-35)."""

    _fields_ = [
        ("doublePrecision", ctypes.c_int),
        ("verbosityLevel", ctypes.c_int),
        ("collectPerKernelTimingInfo", ctypes.c_int),
        ("backend", ctypes.c_char * 20),
        ("numthreads", ctypes.c_int),
        ("useMaterializedJTJ", ctypes.c_int),
        ("useFusedJTJ", ctypes.c_int),
    ]


assert ctypes.sizeof(InitParams) == 44

_lib = None

# (name, restype, argtypes) for every symbol of include/Opt.h and include/opt_amd.h
_VP = ctypes.c_void_p
_SIGNATURES = [
    ("Opt_NewState", _VP, [InitParams]),
    ("Opt_ProblemDefine", _VP, [_VP, ctypes.c_char_p, ctypes.c_char_p]),
    ("Opt_ProblemDelete", None, [_VP, _VP]),
    ("Opt_ProblemPlan", _VP, [_VP, _VP, ctypes.POINTER(ctypes.c_uint)]),
    ("Opt_PlanFree", None, [_VP, _VP]),
    ("Opt_SetSolverParameter", None, [_VP, _VP, ctypes.c_char_p, _VP]),
    ("Opt_ProblemSolve", None, [_VP, _VP, ctypes.POINTER(_VP)]),
    ("Opt_ProblemInit", None, [_VP, _VP, ctypes.POINTER(_VP)]),
    ("Opt_ProblemStep", ctypes.c_int, [_VP, _VP, ctypes.POINTER(_VP)]),
    ("Opt_ProblemCurrentCost", ctypes.c_double, [_VP, _VP]),
    ("OptAMD_PlanUnknownCount", ctypes.c_longlong, [_VP]),
    ("OptAMD_PlanUnknownLayout", ctypes.c_int, [_VP, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong),
                                                ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_int)]),
    ("OptAMD_PlanFamily", ctypes.c_int, [_VP, ctypes.c_char_p, ctypes.c_int]),
    ("OptAMD_ProblemFamily", ctypes.c_int, [_VP, ctypes.c_char_p, ctypes.c_int]),
    ("OptAMD_GenericSignature", ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int]),
    ("OptAMD_EvalJTF", ctypes.c_int, [_VP, _VP, ctypes.POINTER(_VP), _VP, _VP, ctypes.POINTER(ctypes.c_double)]),
    ("OptAMD_ApplyJTJ", ctypes.c_int, [_VP, _VP, ctypes.POINTER(_VP), _VP, _VP, ctypes.POINTER(ctypes.c_double)]),
    ("OptAMD_EvalCost", ctypes.c_double, [_VP, _VP, ctypes.POINTER(_VP)]),
    ("OptAMD_PlanPreconditionerBlocks", ctypes.c_int, [_VP, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                                       ctypes.POINTER(ctypes.c_int)]),
    ("OptAMD_ApplyPreconditioner", ctypes.c_int, [_VP, _VP, ctypes.POINTER(_VP), _VP, _VP]),
    ("OptAMD_PlanEliminated", ctypes.c_int, [_VP, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    ("OptAMD_ApplyReduced", ctypes.c_int, [_VP, _VP, ctypes.POINTER(_VP), _VP, _VP]),
    ("OptAMD_PlanLossGroups", ctypes.c_int, [_VP, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                             ctypes.POINTER(ctypes.c_int)]),
    ("OptAMD_PlanLossGroupEdges", ctypes.c_longlong, [_VP, ctypes.c_int]),
    ("OptAMD_EvalLossWeights", ctypes.c_int, [_VP, _VP, ctypes.POINTER(_VP), ctypes.c_int, _VP]),
    ("OptAMD_TimeApplyJTJ", ctypes.c_double, [_VP, _VP, ctypes.POINTER(_VP), _VP, _VP, ctypes.c_int]),
    ("OptAMD_SetKernelTiming", None, [_VP, ctypes.c_int]),
    ("OptAMD_KernelStat", ctypes.c_int, [_VP, ctypes.c_char_p, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_double)]),
    ("OptAMD_ApplyKernelName", ctypes.c_int, [_VP, ctypes.c_char_p, ctypes.c_int]),
    ("OptAMD_PlanGeneratedForms", ctypes.c_int, [_VP, ctypes.c_char_p, ctypes.c_int]),
    ("OptAMD_KernelReport", ctypes.c_int, [_VP, ctypes.c_char_p, ctypes.c_int]),
    ("OptAMD_PlanStream", _VP, [_VP]),
    ("OptAMD_PlanIterations", ctypes.c_int, [_VP]),
    ("OptAMD_PlanScalars", ctypes.c_int, [_VP, ctypes.POINTER(ctypes.c_double), ctypes.c_int]),
    ("OptAMD_RcclUniqueId", ctypes.c_int, [_VP]),
    ("OptAMD_CommCreateRccl", _VP, [_VP, ctypes.c_int, ctypes.c_int]),
    ("OptAMD_CommDestroy", None, [_VP]),
    ("OptAMD_CommSize", ctypes.c_int, [_VP]),
    ("OptAMD_CommRank", ctypes.c_int, [_VP]),
    ("OptAMD_CommKind", ctypes.c_int, [_VP, ctypes.c_char_p, ctypes.c_int]),
    ("OptAMD_PlanError", ctypes.c_int, [_VP, ctypes.c_char_p, ctypes.c_int]),
    ("OptAMD_LocalGroupCreate", _VP, [ctypes.c_int]),
    ("OptAMD_LocalGroupRank", _VP, [_VP, ctypes.c_int]),
    ("OptAMD_LocalGroupDestroy", None, [_VP]),
    ("OptAMD_PlanHalo", ctypes.c_int, [_VP]),
    ("OptAMD_PlanSetDecomposition", ctypes.c_int, [_VP, _VP, ctypes.c_int, ctypes.c_int]),
    ("OptAMD_PlanJacobianShape", ctypes.c_longlong, [_VP, ctypes.POINTER(ctypes.c_longlong)]),
    ("OptAMD_PlanMaterializedNonzeros", ctypes.c_int, [_VP, ctypes.POINTER(ctypes.c_longlong),
                                                       ctypes.POINTER(ctypes.c_longlong)]),
    ("OptAMD_EvalJacobian", ctypes.c_int, [_VP, _VP, ctypes.POINTER(_VP), _VP, _VP, _VP]),
    ("OptAMD_CsrTranspose", ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_longlong, _VP, _VP, _VP, _VP, _VP,
                                           _VP, ctypes.c_int]),
    ("OptAMD_CsrATA", ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_longlong, _VP, _VP, _VP, _VP, _VP, _VP,
                                     ctypes.POINTER(ctypes.c_longlong), ctypes.c_int]),
    ("OptAMD_CsrSpMV", ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_longlong, _VP, _VP, _VP, _VP, _VP,
                                      ctypes.c_int]),
    ("OptAMD_GenericSource", ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]),
    ("OptAMD_GenericDescribe", ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int]),
    ("OptAMD_GenericPlanCheck", ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int]),
    ("OptAMD_PlanReducedMatrixShape", ctypes.c_int, [_VP, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_int),
                                                     ctypes.POINTER(ctypes.c_longlong)]),
    ("OptAMD_ReducedMatrix", ctypes.c_int, [_VP, ctypes.POINTER(_VP), _VP, _VP, _VP]),
    ("OptAMD_SchurPattern", ctypes.c_int, [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(_VP),
                                           ctypes.POINTER(_VP), ctypes.POINTER(ctypes.c_longlong),
                                           ctypes.POINTER(ctypes.c_longlong), _VP, _VP, _VP, _VP, ctypes.c_char_p,
                                           ctypes.c_int]),
    ("OptAMD_SchurPatternDevice", ctypes.c_int, [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(_VP),
                                                 ctypes.POINTER(_VP), ctypes.POINTER(ctypes.c_longlong),
                                                 ctypes.POINTER(ctypes.c_longlong), _VP, _VP, _VP, _VP, ctypes.c_char_p,
                                                 ctypes.c_int]),
    ("OptAMD_PlanSymbolicInfo", ctypes.c_int, [_VP, ctypes.c_char_p, ctypes.c_int]),
    ("OptAMD_PlanDirectInfo", ctypes.c_int, [_VP, ctypes.c_char_p, ctypes.c_int]),
    ("OptAMD_PlanNormalMatrixShape", ctypes.c_int, [_VP, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_int),
                                                    ctypes.POINTER(ctypes.c_longlong)]),
    ("OptAMD_NormalMatrix", ctypes.c_int, [_VP, ctypes.POINTER(_VP), _VP, _VP, _VP]),
    ("OptAMD_NormalPattern", ctypes.c_int, [ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(_VP), ctypes.POINTER(ctypes.c_int),
                                            ctypes.POINTER(ctypes.c_longlong), ctypes.c_int,
                                            ctypes.POINTER(ctypes.c_longlong), _VP, _VP, _VP, _VP, ctypes.c_char_p,
                                            ctypes.c_int]),
    ("OptAMD_NormalPatternDevice", ctypes.c_int, [ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(_VP),
                                                  ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong), ctypes.c_int,
                                                  ctypes.POINTER(ctypes.c_longlong), _VP, _VP, _VP, _VP, ctypes.c_char_p,
                                                  ctypes.c_int]),
    ("OptAMD_DenseCholesky", ctypes.c_int, [ctypes.c_longlong, _VP, _VP, _VP, _VP, ctypes.c_int,
                                            ctypes.POINTER(ctypes.c_longlong)]),
    ("OptAMD_Covariance", ctypes.c_int, [_VP, _VP, ctypes.POINTER(_VP), ctypes.c_longlong, _VP, _VP, _VP]),
    ("OptAMD_DenseInverseBlocks", ctypes.c_int, [ctypes.c_longlong, _VP, ctypes.c_int, ctypes.c_longlong, _VP, _VP, _VP,
                                                 ctypes.c_int, ctypes.POINTER(ctypes.c_longlong)]),
    ("OptAMD_GenericCompileCheck", ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]),
    ("OptAMD_GenericForms", ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]),
]
EXPORTED_SYMBOLS = [s[0] for s in _SIGNATURES]


def load_library(path: str = None):
    """Load libopt_amd.so (OPT_AMD_LIB overrides the in-tree path, for A/B builds);
    raise if it is missing (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("OPT_AMD_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise OptError(
            f"{path} not found: build the HIP runtime first "
            "(python -c 'import __graft_entry__ as g; g.build()' or `make`)"
        )
    # One HIP runtime per process: PyTorch ships its own libamdhip64.so.7, and whichever
    # copy is loaded first serves both (same soname). Load torch's first when it is
    # installed, so tensors allocated by torch and our kernels share one runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(path)
    for name, res, args in _SIGNATURES:
        fn = getattr(lib, name, None)
        if fn is None:
            if os.path.abspath(path) != os.path.abspath(LIB_PATH):
                continue   # an older A/B build (OPT_AMD_LIB) may predate an extension entry point
            raise OptError(f"{path} does not export {name}")
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _ptr(obj) -> int:
    """Address of a problem parameter: torch tensor, numpy array, ctypes object or int."""
    if obj is None:
        return 0
    if isinstance(obj, int):
        return obj
    if hasattr(obj, "data_ptr"):  # torch.Tensor
        return obj.data_ptr()
    if hasattr(obj, "ctypes"):  # numpy.ndarray
        return obj.ctypes.data
    return ctypes.addressof(obj)


class ParamPack:
    """The void** problemparams array; keeps scalar boxes alive."""

    def __init__(self, values: Sequence):
        self._keep = []
        self.arr = (ctypes.c_void_p * max(1, len(values)))()
        for i, v in enumerate(values):
            if isinstance(v, float):
                box = ctypes.c_float(v)
                self._keep.append(box)
                self.arr[i] = ctypes.addressof(box)
            elif isinstance(v, tuple) and len(v) == 2 and v[0] in ("int", "float", "double"):
                box = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double}[v[0]](v[1])
                self._keep.append(box)
                self.arr[i] = ctypes.addressof(box)
            else:
                self._keep.append(v)
                self.arr[i] = _ptr(v)

    @property
    def ptr(self):
        return ctypes.cast(self.arr, ctypes.POINTER(ctypes.c_void_p))


class OptSolver:
    """One Opt_State + Opt_Problem + Opt_Plan (reference OptSolver, OptSolver.h:46-84)."""

    def __init__(
        self,
        dims: Sequence[int],
        energy_file: str,
        solver_kind: str = "gaussNewtonGPU",
        double_precision: bool = False,
        backend: str = "backend_cuda",
        verbosity: int = 0,
        kernel_timing: bool = False,
        numthreads: int = 1,
        materialized: bool = False,
        fused_jtj: bool = False,
    ):
        self.lib = load_library()
        ip = InitParams()
        ip.doublePrecision = int(double_precision)
        ip.verbosityLevel = verbosity
        ip.collectPerKernelTimingInfo = int(kernel_timing)
        ip.backend = backend.encode()
        ip.numthreads = numthreads
        ip.useMaterializedJTJ = int(materialized)
        ip.useFusedJTJ = int(fused_jtj)
        self.state = self.lib.Opt_NewState(ip)
        if not self.state:
            raise OptError("Opt_NewState failed")
        self.problem = self.lib.Opt_ProblemDefine(self.state, energy_file.encode(), solver_kind.encode())
        if not self.problem:
            raise OptError(f"Opt_ProblemDefine failed for {energy_file}")
        self._dims = (ctypes.c_uint * len(dims))(*dims)
        self.plan = self.lib.Opt_ProblemPlan(self.state, self.problem, self._dims)
        if not self.plan:
            raise OptError("Opt_ProblemPlan failed")
        self.double_precision = double_precision

    # ---- reference API ---------------------------------------------------------
    def set_solver_params(self, params: Dict[str, object]):
        """setAllSolverParameters (OptUtils.h:108-112): ints for the iteration counts."""
        keep = []
        for name, v in params.items():
            box = ctypes.c_int(v) if isinstance(v, int) else ctypes.c_float(v)
            keep.append(box)
            self.lib.Opt_SetSolverParameter(self.state, self.plan, name.encode(), ctypes.addressof(box))

    def solve(self, problem_params: Sequence, solver_params: Optional[Dict[str, object]] = None) -> float:
        if solver_params:
            self.set_solver_params(solver_params)
        pk = ParamPack(problem_params)
        self.lib.Opt_ProblemSolve(self.state, self.plan, pk.ptr)
        return self.cost()

    def init(self, problem_params: Sequence):
        self._pk = ParamPack(problem_params)
        self.lib.Opt_ProblemInit(self.state, self.plan, self._pk.ptr)
        self._raise_plan_error()

    def step(self, problem_params: Optional[Sequence] = None) -> int:
        if problem_params is not None:
            self._pk = ParamPack(problem_params)
        r = self.lib.Opt_ProblemStep(self.state, self.plan, self._pk.ptr)
        self._raise_plan_error()
        return r

    def _raise_plan_error(self):
        """OptAMD_PlanError: a problem the plan met when the arrays were bound."""
        buf = ctypes.create_string_buffer(512)
        if self.lib.OptAMD_PlanError(self.plan, buf, 512) > 0:
            raise OptError(buf.value.decode())

    def profiled_solve(self, problem_params: Sequence) -> List[float]:
        """launchProfiledSolve (OptUtils.h:47-64): cost after Init and after each Step."""
        self.init(problem_params)
        costs = [self.cost()]
        while self.step():
            costs.append(self.cost())
        return costs

    def cost(self) -> float:
        return self.lib.Opt_ProblemCurrentCost(self.state, self.plan)

    # ---- extensions (include/opt_amd.h) ----------------------------------------
    def unknown_count(self) -> int:
        return self.lib.OptAMD_PlanUnknownCount(self.plan)

    def unknown_layout(self):
        """(offsets, elements, channels) of the unknown images' blocks in r / pre / p / Ap
        (OptAMD_PlanUnknownLayout); the blocks differ in length over several index spaces."""
        off, n, ch = (ctypes.c_longlong * 4)(), (ctypes.c_longlong * 4)(), (ctypes.c_int * 4)()
        k = self.lib.OptAMD_PlanUnknownLayout(self.plan, 4, off, n, ch)
        if k < 0:
            raise OptError("OptAMD_PlanUnknownLayout failed")
        return list(off)[:k], list(n)[:k], list(ch)[:k]

    def family(self) -> str:
        buf = ctypes.create_string_buffer(64)
        self.lib.OptAMD_PlanFamily(self.plan, buf, 64)
        return buf.value.decode()

    def eval_jtf(self, problem_params, r, pre) -> float:
        pk = ParamPack(problem_params)
        out = ctypes.c_double()
        if self.lib.OptAMD_EvalJTF(self.state, self.plan, pk.ptr, _ptr(r), _ptr(pre), ctypes.byref(out)):
            self._raise_plan_error()
            raise OptError("OptAMD_EvalJTF failed")
        return out.value

    def apply_jtj(self, problem_params, p, Ap) -> float:
        pk = ParamPack(problem_params)
        out = ctypes.c_double()
        if self.lib.OptAMD_ApplyJTJ(self.state, self.plan, pk.ptr, _ptr(p), _ptr(Ap), ctypes.byref(out)):
            self._raise_plan_error()
            raise OptError("OptAMD_ApplyJTJ failed")
        return out.value

    def preconditioner_blocks(self):
        """(group, first_row) per unknown image and the number of block groups
        (OptAMD_PlanPreconditionerBlocks); ([], [], 0) for a scalar preconditioner."""
        g, fr = (ctypes.c_int * 4)(), (ctypes.c_int * 4)()
        k = self.lib.OptAMD_PlanPreconditionerBlocks(self.plan, 4, g, fr)
        if k < 0:
            raise OptError("OptAMD_PlanPreconditionerBlocks failed")
        if k == 0:
            return [], [], 0
        n = len(self.unknown_layout()[0])
        return list(g)[:n], list(fr)[:n], k

    def apply_preconditioner(self, problem_params, r, z) -> None:
        """z = M^-1 r at the current unknowns (OptAMD_ApplyPreconditioner)."""
        pk = ParamPack(problem_params)
        if self.lib.OptAMD_ApplyPreconditioner(self.state, self.plan, pk.ptr, _ptr(r), _ptr(z)):
            self._raise_plan_error()
            raise OptError("OptAMD_ApplyPreconditioner failed")

    def eliminated(self):
        """0 / 1 per unknown image: whether the plan eliminates it (Eliminate in the energy
        file; OptAMD_PlanEliminated). All 0 on a plan without the statement."""
        f = (ctypes.c_int * 4)()
        k = self.lib.OptAMD_PlanEliminated(self.plan, 4, f)
        if k < 0:
            raise OptError("OptAMD_PlanEliminated failed")
        return list(f)[:k]

    def loss_groups(self):
        """The plan's robust-loss groups, one dict per RobustEnergy statement of the energy file
        (OptAMD_PlanLossGroups): graph id, residuals per edge, kind ("huber" / "cauchy") and the
        graph's edge count. [] on a plan without the statement."""
        g, r, k = (ctypes.c_int * 4)(), (ctypes.c_int * 4)(), (ctypes.c_int * 4)()
        n = self.lib.OptAMD_PlanLossGroups(self.plan, 4, g, r, k)
        if n < 0:
            raise OptError("OptAMD_PlanLossGroups failed")
        return [{"graph": g[i], "residuals": r[i], "kind": ("huber", "cauchy")[k[i]],
                 "edges": self.lib.OptAMD_PlanLossGroupEdges(self.plan, i)} for i in range(n)]

    def loss_weights(self, problem_params, group: int = 0):
        """rho'(s) per edge of one loss group at the bound unknowns, in edge order
        (OptAMD_EvalLossWeights): 1 on a Huber inlier, below 1 where the loss bends. A torch
        tensor on the plan's device; raises on a plan without RobustEnergy or a bad group."""
        import torch
        edges = self.lib.OptAMD_PlanLossGroupEdges(self.plan, group)
        w = torch.empty(max(edges, 1), dtype=torch.float64 if self.double_precision else torch.float32, device="cuda")
        pk = ParamPack(problem_params)
        if self.lib.OptAMD_EvalLossWeights(self.state, self.plan, pk.ptr, group, _ptr(w)):
            self._raise_plan_error()
            raise OptError("OptAMD_EvalLossWeights failed (the plan has no RobustEnergy statement)")
        return w[:max(edges, 0)]

    def apply_reduced(self, problem_params, p, Sp) -> None:
        """Sp = S p, the Schur complement's product at the current unknowns
        (OptAMD_ApplyReduced); raises on a plan without Eliminate."""
        pk = ParamPack(problem_params)
        if self.lib.OptAMD_ApplyReduced(self.state, self.plan, pk.ptr, _ptr(p), _ptr(Sp)):
            self._raise_plan_error()
            raise OptError("OptAMD_ApplyReduced failed (a plan without Eliminate has no reduced system)")

    def reduced_matrix_shape(self):
        """(block rows, block dimension, blocks) of the explicitly formed S once the graphs
        are bound (OptAMD_PlanReducedMatrixShape); None on any other plan, or before."""
        return self._matrix_shape("OptAMD_PlanReducedMatrixShape")

    def reduced_matrix(self, problem_params):
        """S = B - E M^-1 E^T assembled at the bound unknowns, in block-CSR (OptAMD_ReducedMatrix
        on a plan whose energy has ReducedSystem("explicit")): (rowPtr, colInd, val[nnzb, C, C])
        as torch tensors on the plan's device."""
        return self._matrix("OptAMD_ReducedMatrix", self.reduced_matrix_shape, problem_params,
                            "the plan has no explicit reduced system")

    def _matrix_shape(self, fn):
        rows, dim, nnzb = ctypes.c_longlong(), ctypes.c_int(), ctypes.c_longlong()
        k = getattr(self.lib, fn)(self.plan, ctypes.byref(rows), ctypes.byref(dim), ctypes.byref(nnzb))
        if k < 0:
            raise OptError(fn + " failed")
        return (rows.value, dim.value, nnzb.value) if k == 1 else None

    def _matrix(self, fn, shape, problem_params, missing):
        """The assembled block-CSR matrix of an explicit plan: one call of `fn` binds and builds the
        pattern, `shape` sizes the tensors, a second call fills them."""
        import torch
        call = getattr(self.lib, fn)
        pk = ParamPack(problem_params)
        if call(self.plan, pk.ptr, None, None, None):
            self._raise_plan_error()
            raise OptError(f"{fn} failed ({missing})")
        rows, dim, nnzb = shape()
        row_ptr = torch.empty(rows + 1, dtype=torch.int32, device="cuda")
        col_ind = torch.empty(max(nnzb, 1), dtype=torch.int32, device="cuda")
        val = torch.empty((max(nnzb, 1), dim, dim), dtype=torch.float64 if self.double_precision else torch.float32,
                          device="cuda")
        if call(self.plan, pk.ptr, _ptr(row_ptr), _ptr(col_ind), _ptr(val)):
            self._raise_plan_error()
            raise OptError(fn + " failed")
        return row_ptr, col_ind[:nnzb], val[:nnzb]

    def symbolic_info(self):
        """Where the last symbolic phase of the explicit S or H ran (OptAMD_PlanSymbolicInfo): one
        line 'path=device|host reason=default|env|memory pairs= blocks= instances=
        transient_bytes=', '' before the first symbolic phase, -1 on a plan with neither
        ReducedSystem("explicit") nor NormalMatrix("explicit")."""
        buf = ctypes.create_string_buffer(256)
        if self.lib.OptAMD_PlanSymbolicInfo(self.plan, buf, 256) < 0:
            return -1
        return buf.value.decode()

    def direct_info(self):
        """What LinearSolver("cholesky") did on this plan so far (OptAMD_PlanDirectInfo): a dict
        with n, tiles, bytes, factorisations, fallbacks (ints), reason ('none', 'memory' or
        'pivot': the last fall-back's), min_pivot_ratio (float, of the last factorisation),
        covariances (covariance() calls completed) and cov_bytes (the last call's workspace);
        None on a plan without the statement."""
        buf = ctypes.create_string_buffer(256)
        if self.lib.OptAMD_PlanDirectInfo(self.plan, buf, 256) < 0:
            return None
        kv = dict(w.split("=", 1) for w in buf.value.decode().split())
        return {k: (v if k == "reason" else float(v) if k == "min_pivot_ratio" else int(v)) for k, v in kv.items()}

    def covariance(self, problem_params, elements=None, pairs=None):
        """Marginal covariance blocks at the bound unknowns (OptAMD_Covariance): C x C blocks of the
        inverse of the plan's assembled S or H, without LM's diagonal, from the dense Cholesky
        factor of LinearSolver("cholesky"). Default: the diagonal block of every retained
        element; `elements` selects diagonal blocks; `pairs` is a (K, 2) list of (row element,
        column element), numbered as the block rows of normal_matrix() / reduced_matrix().
        Returns a numpy array (K, C, C) in the plan's precision; blocks of excluded or held
        elements are zeros. ValueError on a plan without the statement or a bad index,
        MemoryError when tiles + workspace exceed OPT_AMD_DENSE_MAX_BYTES or the free memory,
        numpy.linalg.LinAlgError (with the row) when a pivot fails."""
        import numpy as np
        import torch
        if self.direct_info() is None:
            raise ValueError('covariance() needs LinearSolver("cholesky") in the energy file, beside '
                             'ReducedSystem("explicit") or NormalMatrix("explicit")')
        pk = ParamPack(problem_params)
        shape = None
        for fn, get in (("OptAMD_NormalMatrix", self.normal_matrix_shape), ("OptAMD_ReducedMatrix", self.reduced_matrix_shape)):
            if getattr(self.lib, fn)(self.plan, pk.ptr, None, None, None) == 0:   # binds and builds the pattern
                shape = get()
                break
        if shape is None:
            self._raise_plan_error()
            raise OptError("covariance: the plan has no assembled matrix")
        rows, dim, _ = shape
        r, c = _block_selection(rows, elements, pairs)
        out = torch.empty((max(len(r), 1), dim, dim), dtype=torch.float64 if self.double_precision else torch.float32,
                          device="cuda")
        e = self.lib.OptAMD_Covariance(self.state, self.plan, pk.ptr, len(r), r.ctypes.data, c.ctypes.data, _ptr(out))
        if e:
            buf = ctypes.create_string_buffer(512)
            self.lib.OptAMD_PlanError(self.plan, buf, 512)
            msg = buf.value.decode() or "OptAMD_Covariance failed"
            raise {1: ValueError, 2: MemoryError, 3: np.linalg.LinAlgError}.get(e, OptError)(msg)
        return out[:len(r)].cpu().numpy()

    def normal_matrix_shape(self):
        """(block rows, block dimension, blocks) of the explicitly formed H = J^T J once the
        graphs are bound (OptAMD_PlanNormalMatrixShape); None on any other plan, or before."""
        return self._matrix_shape("OptAMD_PlanNormalMatrixShape")

    def normal_matrix(self, problem_params):
        """H = J^T J assembled at the bound unknowns, in block-CSR (OptAMD_NormalMatrix on a plan
        whose energy has NormalMatrix("explicit")): (rowPtr, colInd, val[nnzb, C, C]) as torch
        tensors on the plan's device."""
        return self._matrix("OptAMD_NormalMatrix", self.normal_matrix_shape, problem_params,
                            "the plan has no explicit normal matrix")

    def eval_cost(self, problem_params) -> float:
        pk = ParamPack(problem_params)
        c = self.lib.OptAMD_EvalCost(self.state, self.plan, pk.ptr)
        if c == -1.0:   # a cost is >= 0: the call failed (OptAMD_PlanError holds why)
            self._raise_plan_error()
            raise OptError("OptAMD_EvalCost failed")
        return c

    def time_apply(self, problem_params, p, Ap, reps: int) -> float:
        pk = ParamPack(problem_params)
        return self.lib.OptAMD_TimeApplyJTJ(self.state, self.plan, pk.ptr, _ptr(p), _ptr(Ap), reps)

    def set_kernel_timing(self, mode: int):
        self.lib.OptAMD_SetKernelTiming(self.plan, mode)

    def kernel_stat(self, name: str):
        n = ctypes.c_longlong()
        ms = ctypes.c_double()
        ok = self.lib.OptAMD_KernelStat(self.plan, name.encode(), ctypes.byref(n), ctypes.byref(ms)) == 0
        return (n.value, ms.value) if ok else (0, 0.0)

    def apply_kernel_name(self) -> str:
        buf = ctypes.create_string_buffer(64)
        self.lib.OptAMD_ApplyKernelName(self.plan, buf, 64)
        return buf.value.decode()

    def generated_forms(self) -> dict:
        """Which forms of the generated kernels this plan launches (OptAMD_PlanGeneratedForms):
        'apply' / 'jtf' / 'cost' as strings, the grid, the image rows and the strips' row-block
        lengths as ints. OptError on a plan that is not on generated kernels."""
        buf = ctypes.create_string_buffer(512)
        if self.lib.OptAMD_PlanGeneratedForms(self.plan, buf, 512) < 0:
            raise OptError("OptAMD_PlanGeneratedForms: the plan is not on generated kernels")
        return _words(buf.value.decode())

    def kernel_report(self) -> str:
        buf = ctypes.create_string_buffer(1 << 16)
        self.lib.OptAMD_KernelReport(self.plan, buf, 1 << 16)
        return buf.value.decode()

    def stream(self) -> int:
        return self.lib.OptAMD_PlanStream(self.plan) or 0

    def iterations(self) -> int:
        return self.lib.OptAMD_PlanIterations(self.plan)

    def scalars(self, n: int = 256):
        """The plan's device scalar slots after the last call (OptAMD_PlanScalars)."""
        buf = (ctypes.c_double * n)()
        k = self.lib.OptAMD_PlanScalars(self.plan, buf, n)
        return list(buf)[: max(k, 0)]

    def halo(self) -> int:
        return self.lib.OptAMD_PlanHalo(self.plan)

    def set_decomposition(self, comm, y_lo: int, y_hi: int):
        """Own global rows [y_lo, y_hi) of a row-slab decomposition (include/opt_amd.h)."""
        if self.lib.OptAMD_PlanSetDecomposition(self.plan, comm, y_lo, y_hi):
            raise OptError("OptAMD_PlanSetDecomposition failed")

    def jacobian_shape(self):
        """(residual rows, nonzeros) of the materialized J; nnz = -1 if the family has none."""
        rows = ctypes.c_longlong()
        nnz = self.lib.OptAMD_PlanJacobianShape(self.plan, ctypes.byref(rows))
        return rows.value, nnz

    def materialized_nonzeros(self):
        """(nnz J, nnz J^T J) of a materialized plan, None for a matrix-free one."""
        a, b = ctypes.c_longlong(), ctypes.c_longlong()
        if self.lib.OptAMD_PlanMaterializedNonzeros(self.plan, ctypes.byref(a), ctypes.byref(b)):
            return None
        return a.value, b.value

    def eval_jacobian(self, problem_params, rowPtr, colInd, val):
        """J at the current unknowns into device arrays (rowPtr rows+1, colInd/val nnz)."""
        pk = ParamPack(problem_params)
        if self.lib.OptAMD_EvalJacobian(self.state, self.plan, pk.ptr, _ptr(rowPtr), _ptr(colInd), _ptr(val)):
            raise OptError("OptAMD_EvalJacobian failed")

    def close(self):
        if getattr(self, "plan", None):
            self.lib.Opt_PlanFree(self.state, self.plan)
            self.plan = None
        if getattr(self, "problem", None):
            self.lib.Opt_ProblemDelete(self.state, self.problem)
            self.problem = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- device CSR building blocks (include/opt_amd.h) ---------------------------------
def csr_transpose(rows, cols, rowPtr, colInd, val=None):
    """(rowPtrT, colIndT, valT) of a device CSR matrix given as torch tensors."""
    import torch

    lib = load_library()
    nnz = colInd.numel()
    rpT = torch.empty(cols + 1, dtype=torch.int32, device=rowPtr.device)
    ciT = torch.empty(max(nnz, 1), dtype=torch.int32, device=rowPtr.device)
    vT = torch.empty(max(nnz, 1), dtype=val.dtype, device=rowPtr.device) if val is not None else None
    dp = int(val is not None and val.dtype == torch.float64)
    if lib.OptAMD_CsrTranspose(rows, cols, nnz, _ptr(rowPtr), _ptr(colInd), _ptr(val), _ptr(rpT), _ptr(ciT),
                               _ptr(vT), dp):
        raise OptError("OptAMD_CsrTranspose failed")
    return rpT, ciT[:nnz], (vT[:nnz] if vT is not None else None)


def csr_ata(rows, cols, rowPtr, colInd, val):
    """(rowPtrATA, colIndATA, valATA) of A^T A for a device CSR matrix A."""
    import torch

    lib = load_library()
    nnz = colInd.numel()
    dp = int(val.dtype == torch.float64)
    rp = torch.empty(cols + 1, dtype=torch.int32, device=rowPtr.device)
    n = ctypes.c_longlong()
    args = (rows, cols, nnz, _ptr(rowPtr), _ptr(colInd), _ptr(val), _ptr(rp))
    if lib.OptAMD_CsrATA(*args, None, None, ctypes.byref(n), dp):
        raise OptError("OptAMD_CsrATA (pattern) failed")
    ci = torch.empty(max(n.value, 1), dtype=torch.int32, device=rowPtr.device)
    v = torch.empty(max(n.value, 1), dtype=val.dtype, device=rowPtr.device)
    if lib.OptAMD_CsrATA(*args, _ptr(ci), _ptr(v), ctypes.byref(n), dp):
        raise OptError("OptAMD_CsrATA failed")
    return rp, ci[: n.value], v[: n.value]


def csr_spmv(rows, cols, rowPtr, colInd, val, x):
    import torch

    lib = load_library()
    y = torch.empty(rows, dtype=val.dtype, device=x.device)
    dp = int(val.dtype == torch.float64)
    if lib.OptAMD_CsrSpMV(rows, cols, colInd.numel(), _ptr(rowPtr), _ptr(colInd), _ptr(val), _ptr(x), _ptr(y), dp):
        raise OptError("OptAMD_CsrSpMV failed")
    return y


# ---- general energy front end (no device needed) ----------------------------------
def _text_call(fn, *args, cap: int = 1 << 23):
    buf = ctypes.create_string_buffer(cap)
    r = fn(*args, buf, cap)
    return r, buf.value.decode(errors="replace")


def generic_source(energy_file: str, double: bool = False, off32: bool = False) -> str:
    """HIP source the front end generates for `energy_file` (OptAMD_GenericSource); off32:
    the 32-bit gather addressing plans take for arrays below 2 GiB."""
    r, txt = _text_call(load_library().OptAMD_GenericSource, energy_file.encode(), int(double) | (2 if off32 else 0))
    if r < 0:
        raise OptError(txt)
    return txt


def _words(line: str) -> dict:
    """'key=value' words of one report line: integers as int, the rest as str."""
    out = {}
    for w in line.split():
        k, v = w.split("=", 1)
        out[k] = int(v) if v.lstrip("-").isdigit() else v
    return out


def generic_forms(energy_file: str, double: bool = False) -> dict:
    """What the generator emits for `energy_file` beside the gathers (OptAMD_GenericForms):
    has_tiled, tiles_x, tiles_y, has_strip, strip_cols, has_jtf_strip, jtf_strip_cols,
    has_cost_strip, cost_strip_cols, all ints. No device needed."""
    r, txt = _text_call(load_library().OptAMD_GenericForms, energy_file.encode(), int(double), cap=512)
    if r < 0:
        raise OptError(txt)
    return _words(txt)


def generic_describe(energy_file: str) -> List[str]:
    """Residual templates of `energy_file`: '<centred|graphK> <n unknowns> <expression>'."""
    r, txt = _text_call(load_library().OptAMD_GenericDescribe, energy_file.encode())
    if r < 0:
        raise OptError(txt)
    return txt.splitlines()


def generic_signature(energy_file: str) -> str:
    """Structural signature of the lowered energy (OptAMD_GenericSignature)."""
    r, txt = _text_call(load_library().OptAMD_GenericSignature, energy_file.encode())
    if r < 0:
        raise OptError(txt)
    return txt


def generic_plan_check(energy_file: str) -> str:
    """The shape checks Opt_ProblemPlan makes before it asks for a device
    (OptAMD_GenericPlanCheck): '' if the plan would accept the energy, else its refusal."""
    r, txt = _text_call(load_library().OptAMD_GenericPlanCheck, energy_file.encode())
    if r < 0:
        raise OptError(txt)
    return txt if r else ""


def schur_pattern(n_eliminated: int, n_retained: int, lists, device: bool = False):
    """Symbolic phase of the explicitly formed Schur complement on the host
    (OptAMD_SchurPattern), or with device=True by the device builder a plan uses
    (OptAMD_SchurPatternDevice: the same arrays element for element). lists: (eliminated vertex
    per edge, retained vertex per edge) pairs.
    Returns (counts {instances, pairs, blocks}, rowPtr, colInd, pairPtr, pairs[npairs, 2])."""
    import numpy as np
    lib = load_library()
    fn = lib.OptAMD_SchurPatternDevice if device else lib.OptAMD_SchurPattern
    ev = [np.ascontiguousarray(a, np.int32) for a, _ in lists]
    rv = [np.ascontiguousarray(b, np.int32) for _, b in lists]
    k = len(lists)
    evp = (_VP * max(k, 1))(*[a.ctypes.data for a in ev])
    rvp = (_VP * max(k, 1))(*[a.ctypes.data for a in rv])
    ne = (ctypes.c_longlong * max(k, 1))(*[len(a) for a in ev])
    counts = (ctypes.c_longlong * 3)()
    buf = ctypes.create_string_buffer(512)
    if fn(n_eliminated, n_retained, k, evp, rvp, ne, counts, None, None, None, None, buf, 512):
        raise OptError(buf.value.decode())
    nq, npairs, nnzb = list(counts)
    row_ptr, col_ind = np.zeros(n_retained + 1, np.int32), np.zeros(nnzb, np.int32)
    pair_ptr, pairs = np.zeros(nnzb + 1, np.int32), np.zeros((npairs, 2), np.int32)
    if fn(n_eliminated, n_retained, k, evp, rvp, ne, counts, row_ptr.ctypes.data, col_ind.ctypes.data,
          pair_ptr.ctypes.data, pairs.ctypes.data, buf, 512):
        raise OptError(buf.value.decode())
    return {"instances": nq, "pairs": npairs, "blocks": nnzb}, row_ptr, col_ind, pair_ptr, pairs


def normal_pattern(n_vertices: int, lists, graph_edges=None, device: bool = False):
    """Symbolic phase of the explicitly formed J^T J on the host (OptAMD_NormalPattern), or with
    device=True by the device builder a plan uses (OptAMD_NormalPatternDevice). lists:
    one vertex array per slot over the unknowns' space, or (graph, vertex array) pairs with
    graph_edges the edge count of each graph. Returns (counts {instances, pairs, blocks},
    rowPtr, colInd, pairPtr, pairs[npairs, 2])."""
    import numpy as np
    lib = load_library()
    fn = lib.OptAMD_NormalPatternDevice if device else lib.OptAMD_NormalPattern
    if graph_edges is None:
        lists = [(0, v) for v in lists]
        graph_edges = [len(lists[0][1])] if lists else []
    vs = [np.ascontiguousarray(v, np.int32) for _, v in lists]
    k, ng = len(lists), len(graph_edges)
    vp = (_VP * max(k, 1))(*[a.ctypes.data for a in vs])
    lg = (ctypes.c_int * max(k, 1))(*[g for g, _ in lists])
    ge = (ctypes.c_longlong * max(ng, 1))(*graph_edges)
    counts = (ctypes.c_longlong * 3)()
    buf = ctypes.create_string_buffer(512)
    if fn(n_vertices, k, vp, lg, ge, ng, counts, None, None, None, None, buf, 512):
        raise OptError(buf.value.decode())
    nq, npairs, nnzb = list(counts)
    row_ptr, col_ind = np.zeros(n_vertices + 1, np.int32), np.zeros(nnzb, np.int32)
    pair_ptr, pairs = np.zeros(nnzb + 1, np.int32), np.zeros((npairs, 2), np.int32)
    if fn(n_vertices, k, vp, lg, ge, ng, counts, row_ptr.ctypes.data, col_ind.ctypes.data,
          pair_ptr.ctypes.data, pairs.ctypes.data, buf, 512):
        raise OptError(buf.value.decode())
    return {"instances": nq, "pairs": npairs, "blocks": nnzb}, row_ptr, col_ind, pair_ptr, pairs


def dense_cholesky(A, b, L=None, x=None):
    """Dense Cholesky factorisation and solve on the device (OptAMD_DenseCholesky): A (n x n,
    symmetric positive definite) and b (n) as float32 or float64 numpy arrays (A's dtype decides).
    Returns (L, x, info): the lower-triangular factor, the solution of A x = b and -1; where the
    pivot of a row fails, info is that row and L and x (the caller's contiguous arrays of A's
    dtype where given, else zeros) are left untouched."""
    import numpy as np
    dt = np.float64 if np.asarray(A).dtype == np.float64 else np.float32
    A = np.ascontiguousarray(A, dt)
    b = np.ascontiguousarray(b, dt)
    n = A.shape[0]
    if A.shape != (n, n) or b.shape != (n,) or n < 1:
        raise OptError("dense_cholesky: A must be n x n and b of length n, n >= 1")
    L = np.zeros((n, n), dt) if L is None else L
    x = np.zeros(n, dt) if x is None else x
    for o, shape in ((L, (n, n)), (x, (n,))):
        if o.dtype != dt or o.shape != shape or not o.flags.c_contiguous:
            raise OptError("dense_cholesky: L and x must be contiguous arrays of A's dtype and shape")
    info = ctypes.c_longlong(-1)
    if load_library().OptAMD_DenseCholesky(n, A.ctypes.data, b.ctypes.data, L.ctypes.data, x.ctypes.data,
                                           int(dt == np.float64), ctypes.byref(info)):
        raise OptError("OptAMD_DenseCholesky: invalid arguments, or the matrix does not fit the device")
    return L, x, int(info.value)


def _block_selection(n_elements, elements, pairs):
    """(row elements, column elements) as int32 arrays for covariance() / dense_inverse_blocks():
    `pairs` (K, 2), else the diagonal blocks of `elements`, else of every element. ValueError on
    an index outside [0, n_elements)."""
    import numpy as np
    if pairs is not None and elements is not None:
        raise ValueError("give elements or pairs, not both")
    if pairs is not None:
        pq = np.asarray(pairs, np.int64).reshape(-1, 2)
    else:
        e = np.arange(n_elements) if elements is None else np.asarray(elements, np.int64).reshape(-1)
        pq = np.stack([e, e], axis=1)
    if pq.size and (pq.min() < 0 or pq.max() >= n_elements):
        raise ValueError(f"element index out of range: the matrix has {n_elements} elements")
    return np.ascontiguousarray(pq[:, 0], np.int32), np.ascontiguousarray(pq[:, 1], np.int32)


def dense_inverse_blocks(A, C, elements=None, pairs=None, out=None):
    """Blocks of A^-1 on the device from the dense Cholesky factor (OptAMD_DenseInverseBlocks; the
    kernels behind OptSolver.covariance): A (n x n, symmetric positive definite, float32 or
    float64 numpy) cut into elements of C unknowns. The selection as in covariance(). Returns
    (blocks (K, C, C), info): info is -1, or the first row whose pivot failed, and then blocks (the
    caller's `out` where given, else zeros) is untouched. ValueError for n no multiple of C or an
    index out of range, before any launch; MemoryError when the storage does not fit the device."""
    import numpy as np
    dt = np.float64 if np.asarray(A).dtype == np.float64 else np.float32
    A = np.ascontiguousarray(A, dt)
    n = A.shape[0]
    if A.ndim != 2 or A.shape != (n, n) or n < 1:
        raise ValueError("dense_inverse_blocks: A must be n x n, n >= 1")
    if not 1 <= C <= 64 or n % C:
        raise ValueError(f"dense_inverse_blocks: n = {n} must be a multiple of C = {C}, 1 <= C <= 64")
    r, c = _block_selection(n // C, elements, pairs)
    out = np.zeros((len(r), C, C), dt) if out is None else out
    if out.dtype != dt or out.shape != (len(r), C, C) or not out.flags.c_contiguous:
        raise ValueError("dense_inverse_blocks: out must be a contiguous (K, C, C) array of A's dtype")
    info = ctypes.c_longlong(-1)
    if load_library().OptAMD_DenseInverseBlocks(n, A.ctypes.data, C, len(r), r.ctypes.data, c.ctypes.data, out.ctypes.data,
                                                int(dt == np.float64), ctypes.byref(info)):
        raise ValueError("OptAMD_DenseInverseBlocks: invalid arguments")
    if info.value == -2:
        raise MemoryError("OptAMD_DenseInverseBlocks: the tiles and the selection's workspace do not fit the device")
    return out, int(info.value)


def problem_family(energy_file: str, solver_kind: str = "gaussNewtonGPU") -> str:
    """Kernel family Opt_ProblemDefine picks for `energy_file` (OptAMD_ProblemFamily):
    a hand-written family only if the file lowers to exactly its residual templates."""
    lib = load_library()
    ip = InitParams()
    ip.backend = b"backend_cuda"
    st = lib.Opt_NewState(ip)
    pr = lib.Opt_ProblemDefine(st, energy_file.encode(), solver_kind.encode())
    if not pr:
        raise OptError(f"Opt_ProblemDefine refused {energy_file}")
    buf = ctypes.create_string_buffer(64)
    lib.OptAMD_ProblemFamily(pr, buf, 64)
    lib.Opt_ProblemDelete(st, pr)
    return buf.value.decode()


def generic_compile_check(energy_file: str, double: bool = False) -> None:
    """Compile the generated source for gfx950 with hiprtc; raise with the log on error."""
    r, txt = _text_call(load_library().OptAMD_GenericCompileCheck, energy_file.encode(), int(double))
    if r != 0:
        raise OptError(txt)
