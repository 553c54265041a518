"""Float64 reference for RobustEnergy (Robust losses) — a test helper, CPU only.

Built on oracle.examples_ad.Model without touching oracle/: robustify() wraps one term of a
model as f * sqrt(rho'(sum f^2)).detach(), so that Model.residuals() / Model.jacobian() are
those of the reweighted problem (f~ = w f, J~ = w J, w held constant: jacfwd sees no
dependence through the detached weight, as intrinsic_image_decomposition's L_p weight), and
keeps the raw term for s, rho and rho'. cost() is the robust cost 1/2 sum rho(s) + 1/2 sum
r^2 over the plain terms. solve() is oracle.examples_ad.solve with two changes: cost is the
robust cost, and the model cost (which only LM reads) is
1/2 sum_blocks [rho(s) - rho'(s) s + sum_k (f~_k + J~_k d)^2] + the plain terms.

Ceres' definitions on s: huber rho = s (s <= a^2) else 2 a sqrt(s) - a^2; cauchy
rho = a^2 log(1 + s / a^2)."""
import ctypes

import numpy as np

from oracle import examples_ad as ad


def rho(kind, a, s):
    s = np.asarray(s, np.float64)
    if kind == "huber":
        return np.where(s <= a * a, s, 2.0 * a * np.sqrt(s) - a * a)
    assert kind == "cauchy"
    return a * a * np.log1p(s / (a * a))


def rho1(kind, a, s):
    s = np.asarray(s, np.float64)
    if kind == "huber":
        return np.where(s <= a * a, 1.0, a / np.sqrt(np.maximum(s, 1e-300)))
    assert kind == "cauchy"
    return 1.0 / (1.0 + s / (a * a))


class RobustModel(ad.Model):
    """An ad.Model some of whose terms carry a loss: .loss = [{term, fn (raw), kind, a}], `a`
    read at every evaluation (a test may change it between two steps)."""

    def __init__(self, model):
        self.__dict__.update(model.__dict__)
        self.terms = list(model.terms)
        self.x = dict(model.x)
        self.loss = []

    def _rows(self, term_index):
        r0 = 0
        for t, (_, args, k) in enumerate(self.terms):
            n = len(args[0][2]) * k
            if t == term_index:
                return r0, r0 + n
            r0 += n
        raise IndexError(term_index)

    def s(self, group=0):
        """s = sum_k f_k^2 per edge of a loss group, from the raw term."""
        import torch
        L = self.loss[group]
        _, args, _ = self.terms[L["term"]]
        f = torch.vmap(L["fn"])(*self._gather(args))
        return (f * f).reshape(len(args[0][2]), -1).sum(1).numpy()

    def loss_rho1(self, group=0):
        L = self.loss[group]
        return rho1(L["kind"], L["a"], self.s(group))

    def plain_mask(self):
        """True on the residual rows of the plain terms."""
        m = np.ones(sum(len(a[0][2]) * k for _, a, k in self.terms), bool)
        for L in self.loss:
            lo, hi = self._rows(L["term"])
            m[lo:hi] = False
        return m

    def cost(self):
        F = self.residuals()[self.plain_mask()]
        c = 0.5 * float(F @ F)
        for g, L in enumerate(self.loss):
            c += 0.5 * float(rho(L["kind"], L["a"], self.s(g)).sum())
        return c

    def model_constant(self):
        """1/2 sum_blocks (rho(s) - rho'(s) s): what the weighted model's 1/2 |F~ + J~ d|^2 lacks."""
        c = 0.0
        for g, L in enumerate(self.loss):
            s = self.s(g)
            c += 0.5 * float((rho(L["kind"], L["a"], s) - rho1(L["kind"], L["a"], s) * s).sum())
        return c


def robustify(model, term_index, kind, a):
    """`model` (an ad.Model or a RobustModel) with term `term_index` under the loss; returns a
    RobustModel sharing nothing mutable with `model`."""
    import torch
    m = model if isinstance(model, RobustModel) else RobustModel(model)
    fn, args, k = m.terms[term_index]
    L = {"term": term_index, "fn": fn, "kind": kind, "a": float(a)}

    def weighted(*g):
        f = fn(*g)
        s = (f * f).sum()
        a_ = L["a"]
        if kind == "huber":
            safe = torch.where(s <= a_ * a_, torch.ones_like(s), s)
            w2 = torch.where(s <= a_ * a_, torch.ones_like(s), a_ / torch.sqrt(safe))
        else:
            w2 = 1.0 / (1.0 + s / (a_ * a_))
        return f * torch.sqrt(w2).detach()

    m.terms[term_index] = (weighted, args, k)
    m.loss.append(L)
    return m


def solve(model, n_iter, l_iter, lm=False, use_pre=True, corrected=True, **kw):
    """oracle.examples_ad.solve (the same C loop through the same ctypes structs) with the robust
    cost and the robust model cost; corrected=False leaves the rho - rho' s term out of the
    model cost (what a solver that only reweights would compare). Returns the costs after
    init and after each step."""
    lib = ad._c.load()
    lib.oracle_solve_f64.restype = ctypes.c_int
    lib.oracle_solve_f64.argtypes = [ctypes.POINTER(ad._Problem), ctypes.c_int, ctypes.POINTER(ad._Params), ad._D]
    n = model.n
    st = {"J": None, "prev": None}

    def arr(ptr):
        return np.ctypeslib.as_array(ptr, shape=(n,))

    def J():
        if st["J"] is None:
            st["J"] = model.jacobian()
        return st["J"]

    def cost(_):
        return model.cost()

    def jtf(_, r, diag):
        st["J"] = None
        Jm = J()
        arr(r)[:] = -(Jm.T @ model.residuals())
        arr(diag)[:] = model.diag_access

    def apply(_, p, Ap):
        pv = arr(p).copy()
        out = J().T @ (J() @ pv)
        arr(Ap)[:] = out
        return float(pv @ out)

    def model_cost(_, d):
        m = model.residuals() + J() @ arr(d)
        return 0.5 * float(m @ m) + (model.model_constant() if corrected else 0.0)

    def update(_, d):
        model.set(model.get() + arr(d))
        st["J"] = None

    def save(_):
        st["prev"] = model.get()

    def revert(_):
        model.set(st["prev"])
        st["J"] = None

    act = np.ones(n, np.uint8)
    cbs = [ad._COST(cost), ad._JTF(jtf), ad._APPLY(apply), ad._MODEL(model_cost), ad._UPD(update), ad._VOID(save),
           ad._VOID(revert)]
    P = ad._Problem(n, act.ctypes.data, int(use_pre), None, *cbs, None, None)
    sp = ad.default_params(n_iter, l_iter, **kw)
    costs = np.zeros(n_iter + 1)
    k = lib.oracle_solve_f64(ctypes.byref(P), int(lm), ctypes.byref(sp), costs.ctypes.data_as(ad._D))
    return costs[: k + 1]
