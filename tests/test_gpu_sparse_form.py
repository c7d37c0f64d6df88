"""-m gpu: the sparse quadratic form transpose(x)*Q*x with a sparse Q Parameter (pmt_sparse_form_f64, csrc/sparse_form.hip).
Through the C ABI: guard words around every output, the output bit for bit against the Python restatement of the contract
(sparse_form_util.restate, proven against the oracle on the CPU) at the wave and workgroup edges, and against the dense node
pmt_quad_form_f64 on the densified matrix without tolerance.  Through Model: the bare record ("canonical-sparse-form") small and beyond
the small plan, both hand-offs, as a constraint, solve after solve; sums with a form ("canonical-sparse-sum") bit for bit against
sparse_sum_util's restatement with the form as a block without linear terms; one solved QP against its dense statement."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sp = pytest.importorskip("scipy.sparse")

import gpu_util as g  # noqa: E402
import parametron_jl_amd as P  # noqa: E402
import sparse_form_util as U  # noqa: E402
import sparse_gram_util as SG  # noqa: E402
from parametron_jl_amd import _lib  # noqa: E402
from sparse_sum_util import Term  # noqa: E402

QT = _lib.QT
POISON = -7


def dev_u32(a):
    """device copy of a uint32 table (never empty: a null table pointer is an error of its own)"""
    raw = np.frombuffer(np.ascontiguousarray(a, dtype=np.uint32).tobytes() + b"\0" * 8, dtype=np.uint8)
    return torch.from_numpy(raw.copy()).to(g.DEV)


class Abi:
    """pmt_sparse_form_f64 on the library's own tables for one pattern.  The output terms and the constant sit between guard words (`odd`:
    an odd number of them in front, so that the output's base is 8 mod 16) and start out poisoned; nzval and the tables are device copies
    that the call must leave as they are."""

    def __init__(self, Q, xvar, varmap, odd=False):
        g.lib()
        self.Q = Q = U.csc(Q)
        self.T = T = U.form_tables(Q)
        self.tabs = {k: dev_u32(getattr(T, k)) for k in T.TABLES}
        self.nz = g.to_dev(np.concatenate([Q.data, [0.0]]))
        self.dx = g.to_dev(np.asarray(xvar, dtype=np.int64) if len(xvar) else np.zeros(1, dtype=np.int64))
        self.dvm = g.to_dev(np.asarray(varmap, dtype=np.int64)) if varmap is not None else None
        self.G = G = 5 if odd else 4
        self.oq = torch.full((2 * G + 3 * T.nq,), POISON, dtype=torch.int64, device=g.DEV)
        self.oc = torch.full((2 * G + 1,), POISON, dtype=torch.int64, device=g.DEV)
        assert (self.oq.data_ptr() + 8 * G) % 16 == (8 if odd else 0)

    def set_values(self, v):
        self.nz[:len(v)] = torch.from_numpy(np.asarray(v, dtype=np.float64)).to(g.DEV)       # in place: the same device buffer

    def run(self, moi, const=True):
        G, T = self.G, self.T
        base = lambda t: C.c_void_p(t.data_ptr() + 8 * G)                 # noqa: E731
        self.oq.fill_(POISON)
        self.oc.fill_(POISON)
        before = [t.clone() for t in self.tabs.values()] + [self.nz.clone()]
        g.call("pmt_sparse_form_f64", g.ptr(self.nz), *[g.ptr(self.tabs[k]) for k in ("src_a", "src_b", "pair_j", "pair_k")], T.nq, g.ptr(self.dx), moi,
               g.ptr(self.dvm) if moi else None, base(self.oq), base(self.oc) if const else None, g.stream())
        torch.cuda.synchronize()
        for a, b in zip(before, list(self.tabs.values()) + [self.nz]):
            assert torch.equal(a, b), "an input was written"
        hq, hc = self.oq.cpu().numpy(), self.oc.cpu().numpy()
        assert np.all(hq[:G] == POISON) and np.all(hq[G + 3 * T.nq:] == POISON), "a guard word of the terms was overwritten"
        assert np.all(hc[:G] == POISON) and np.all(hc[G + 1:] == POISON), "a guard word of the constant was overwritten"
        if const:
            c = hc[G:G + 1].view(np.float64)
            assert c[0] == 0.0 and not np.signbit(c[0])
        else:
            assert hc[G] == POISON, "the constant was written though out_const is null"
        return hq[G:G + 3 * T.nq].copy().view(QT)


def make_vars(rng, n, extra=5):
    """a strictly increasing x among n + extra variables and a permuting, shifted index map"""
    xvar = np.sort(rng.choice(np.arange(1, n + extra + 1), n, replace=False)).astype(np.int64)
    varmap = (rng.permutation(n + extra) + 1 + 3).astype(np.int64)
    return xvar, varmap


# ---- 1. the kernel through the C ABI
EDGES = [1, 63, 64, 65, 255, 256, 257, 513]


@pytest.mark.parametrize("nq", EDGES)
def test_wave_and_workgroup_edges_bit_for_bit(nq):
    """n <= 64 mixed patterns (both / upper-only / lower-only / diagonal pairs side by side in every wave, values with 0.0 and -0.0) with
    exactly nq pairs; moi 0 and 1, an identity and a permuted index map, the output base at 0 and at 8 mod 16, out_const given and null;
    then the values changed in place: new coefficients, the same index words"""
    rng = np.random.default_rng(100 + nq)
    n = 8 if nq == 1 else 40
    Q = U.with_nq(nq, n, rng)
    tabs = U.tables(Q)
    kinds = {(a != U.NONE, b != U.NONE, j == k) for j, k, a, b in zip(*tabs)}
    if nq >= 63:
        assert kinds == {(True, True, False), (True, False, False), (False, True, False), (True, False, True)}
        first = {(a != U.NONE, b != U.NONE, j == k) for j, k, a, b in zip(*[t[:64] for t in tabs])}
        assert first == kinds                                              # every mix inside one wave
    xvar, perm = make_vars(rng, n)
    ident = np.arange(1, n + 6, dtype=np.int64)
    for odd in (False, True):
        for varmap in (ident, perm):
            abi = Abi(Q, xvar, varmap, odd=odd)
            assert abi.T.nq == nq
            for moi in (0, 1):
                for const in (True, False):
                    got = abi.run(moi, const)
                    g.assert_terms_equal(got, U.restate(Q, xvar, moi, varmap, tabs=tabs))
            v2 = U.values(rng, Q.nnz)
            abi.set_values(v2)
            again = abi.run(1)
            g.assert_terms_equal(again, U.restate(Q, xvar, 1, varmap, nzval=v2, tabs=tabs))
            assert np.array_equal(again["row"], got["row"]) and np.array_equal(again["col"], got["col"])
            assert nq < 8 or not g.same_bits(again["coeff"], got["coeff"])


@pytest.mark.parametrize("kind", [k for k in U.KINDS if k != "none"])
def test_pattern_classes_bit_for_bit(kind):
    rng = np.random.default_rng(7)
    n = 33
    Q = U.pattern(kind, n, rng)
    xvar, varmap = make_vars(rng, n)
    for moi in (1, 0):
        g.assert_terms_equal(Abi(Q, xvar, varmap, odd=moi == 0).run(moi), U.restate(Q, xvar, moi, varmap))


def test_no_term_writes_the_constant_only_or_nothing():
    Q = sp.csc_matrix((5, 5), dtype=np.float64)
    xvar, varmap = make_vars(np.random.default_rng(1), 5)
    abi = Abi(Q, xvar, varmap)
    assert abi.T.nq == 0
    assert len(abi.run(1, const=True)) == 0 and len(abi.run(1, const=False)) == 0 and len(abi.run(0, const=True)) == 0


# ---- 2. against the dense node, without tolerance
def test_equals_the_dense_form_node_on_the_densified_matrix():
    """n = 48, values without -0.0: at its pairs the sparse node's coefficients ARE pmt_quad_form_f64's on the densified matrix — the sum of
    the same two numbers (a structural zero adds + 0.0, which changes no value but -0.0) — and the dense node's other coefficients are 0.0"""
    rng = np.random.default_rng(48)
    n = 48
    Q = U.pattern("mixed", n, rng, density=0.1, zeros=False)
    Q.data[::7] = 0.0                                                      # stored zeros: the terms exist
    xvar, varmap = make_vars(rng, n)
    dense = g.colmajor(Q.toarray())
    dx, dvm = g.to_dev(xvar), g.to_dev(varmap)
    nq = n * (n + 1) // 2
    for moi in (1, 0):
        oq = g.empty_terms(nq, QT)
        g.call("pmt_quad_form_f64", g.ptr(dense), n, n, g.ptr(dx), moi, g.ptr(dvm) if moi else None, 1.0, g.ptr(oq), None, None, None, g.stream())
        dq = g.terms_to_host(oq, nq, QT)
        got = Abi(Q, xvar, varmap).run(moi)
        at = {(int(r), int(c)): t for t, (r, c) in enumerate(zip(dq["row"], dq["col"]))}
        hit = np.array([at[(int(r), int(c))] for r, c in zip(got["row"], got["col"])])
        assert len(set(hit.tolist())) == len(got) and np.all(np.diff(hit) > 0)          # the same (j, k) order
        assert g.same_bits(dq["coeff"][hit], got["coeff"])
        rest = np.ones(nq, dtype=bool)
        rest[hit] = False
        assert rest.any() and np.all(dq["coeff"][rest] == 0.0)


# ---- 3. through Model
class Perm(P.MockOptimizer):
    def copy_to(self, backend):
        out = super().copy_to(backend)
        out["variables"] = out["variables"][::-1].copy() + 10
        return out


def _q40(seed=40, n=40, per_row=5):
    """n = 40, about 5 entries per row, unsymmetric: pairs stored twice, once above, once below, and most of the diagonal"""
    rng = np.random.default_rng(seed)
    M = rng.random((n, n)) < (per_row - 1) / n
    M |= np.eye(n, dtype=bool) & (rng.random((n, n)) < 0.9)
    r, c = np.nonzero(M)
    return U.from_entries(n, r, c, SG.signed_values(rng, len(r)))


class Problem:
    """an objective (or constraint) built from transpose(x)*Q*x with host-updated sparse Parameters Q, R (fixed patterns)"""

    def __init__(self, kind="bare", optimizer=None, extra=2, as_constraint=False, dense=False, n=40, **kw):
        rng = np.random.default_rng(3)
        self.kind, self.n = kind, n
        self.Q, self.R = _q40(40, n), _q40(41, n)
        m = 60
        self.Cs = SG.random_csc(rng, m, n, 0.1)
        self.part = np.array([1, 2, 5, 11, 12, n - 1])
        self.st = st = {"Q": self.Q.data.copy(), "R": self.R.data.copy(), "C": self.Cs.data.copy(), "d": SG.signed_values(rng, m), "w": 1.5, "lam": 0.25,
                        "c": SG.signed_values(rng, n), "s": 0.75}
        self.model = model = P.Model(optimizer or Perm(), **kw)
        pre = [P.Variable(model) for _ in range(extra)]                    # x does not start at Variable 1
        x = [P.Variable(model) for _ in range(n)]
        self.x = x
        self.xvar = np.arange(extra + 1, extra + n + 1, dtype=np.int64)
        self.nvars = len(pre) + n

        def sparse(key, M):
            def upd(Mm):
                Mm.data[:] = st[key]
            if dense:
                return P.Parameter(lambda: self.current(key).toarray(), model)
            return P.Parameter(upd, M.copy(), model)
        par = lambda key: P.Parameter(lambda: st[key], model)             # noqa: E731
        self.Qp = Qp = sparse("Q", self.Q)
        form = P.transpose(x) * Qp * x
        if kind == "bare":
            expr = form
        elif kind == "bilinear":
            expr = P.bilinear(x, Qp, x)
        elif kind == "weighted":
            expr = par("w") * form
        elif kind == "qp":
            expr = 0.5 * form + P.dot(par("c"), x) + par("s")
        elif kind == "block":
            r = sparse("C", self.Cs) * x - par("d")
            expr = P.dot(r, r) + form
        elif kind == "ridge":
            expr = form + par("lam") * P.dot(x, x)
        elif kind == "two":
            expr = form + par("w") * (P.transpose(x) * sparse("R", self.R) * x)
        elif kind == "part":
            u = [x[i] for i in self.part]
            expr = form - 0.5 * P.dot(u, u)
        elif kind == "dense block beside":
            A = P.Parameter(lambda: np.ones((5, n)), model)
            r2 = A * x
            expr = form + P.dot(r2, r2)
        elif kind == "dense form beside":
            expr = form + P.transpose(x) * P.Parameter(lambda: np.ones((n, n)), model) * x
        if as_constraint:
            P.objective(model, P.Minimize, P.dot(par("c"), x))
            model.add_nonpositive_constraint(expr)                        # (P.constraint subtracts its right-hand side: a sum, not the bare node)
        else:
            P.objective(model, P.Minimize, expr)

    def current(self, key):
        M = {"Q": self.Q, "R": self.R, "C": self.Cs}[key].copy()
        M.data[:] = self.st[key]
        return M

    def new_values(self, seed):
        rng = np.random.default_rng(seed)
        st = self.st
        for k in ("Q", "R", "C", "d", "c"):
            st[k] = SG.signed_values(rng, len(st[k]))
        st["w"], st["lam"], st["s"] = float(rng.uniform(-2, 2)), float(rng.uniform(0.1, 2)), float(rng.standard_normal())

    def terms(self):
        """the sum in plain data, in expression order, at the current values (the scalar weights are device Parameters: weight=)"""
        st = self.st
        fq = lambda **kw: U.FormTerm(self.current("Q"), **kw)              # noqa: E731
        return {"weighted": lambda: [fq(weight=st["w"])],
                "qp": lambda: [fq(scale=0.5), Term("linear", v=st["c"]), Term("constant", value=st["s"])],
                "block": lambda: [Term("block", Cs=self.current("C"), d=st["d"], sign=-1), fq()],
                "ridge": lambda: [fq(), Term("diag", weight=st["lam"])],
                "two": lambda: [fq(), U.FormTerm(self.current("R"), weight=st["w"])],
                "part": lambda: [fq(), Term("diag", cols=self.part, scale=-0.5)]}[self.kind]()

    def solved(self, record=None):
        P.solve(self.model)
        f = (record or self.model.objective).f
        return f.quadratic_terms.copy(), f.affine_terms.copy(), float(f.constant)


MODELS = {"small, auto": ({}, True), "small, canonical": ({"quadratic_mode": "canonical"}, True), "graph, auto": ({"use_graph": True}, False),
          "graph, canonical": ({"quadratic_mode": "canonical", "use_graph": True}, False)}


@pytest.mark.parametrize("flavour", list(MODELS))
@pytest.mark.parametrize("kind", ["bare", "bilinear"])
def test_bare_objective_bit_for_bit_solve_after_solve(kind, flavour):
    kw, small = MODELS[flavour]
    prob = Problem(kind, **kw)
    try:
        nbytes = []
        for it in range(3):
            if it:
                prob.new_values(50 + it)
            quad, lin, const = prob.solved()
            assert prob.model.objective.mode == "canonical-sparse-form" and prob.model._small == small
            varmap = np.asarray(prob.model.model_var_to_optimizer, dtype=np.int64)
            assert np.array_equal(varmap, np.arange(prob.nvars, 0, -1) + 10)
            g.assert_terms_equal(quad, U.restate(prob.current("Q"), prob.xvar, 1, varmap))
            assert len(lin) == 0 and const == 0.0
            nbytes.append(prob.model.device().bytes_allocated())
        assert len(set(nbytes)) == 1, "plan memory grew across solves: %r" % (nbytes,)
    finally:
        prob.model.close()


def test_a_changed_pattern_raises_dimension_mismatch():
    st = {"Q": _q40()}
    model = P.Model(Perm())
    try:
        x = [P.Variable(model) for _ in range(40)]
        Qp = P.Parameter(lambda: st["Q"], model)
        P.objective(model, P.Minimize, P.transpose(x) * Qp * x)
        P.solve(model)
        assert model.objective.mode == "canonical-sparse-form"
        st["Q"] = sp.csc_matrix(_q40().toarray() + 3.0 * np.eye(40, k=9))
        with pytest.raises(_lib.DimensionMismatch, match="pattern"):
            P.solve(model)
    finally:
        model.close()


@pytest.mark.parametrize("flavour", ["small, auto", "graph, canonical"])
def test_as_a_constraint_record(flavour):
    kw, _ = MODELS[flavour]
    prob = Problem("bare", as_constraint=True, **kw)
    try:
        con = list(prob.model.constraints)[0]
        for it in range(2):
            if it:
                prob.new_values(70)
            quad, lin, const = prob.solved(con)
            assert con.mode == "canonical-sparse-form"
            varmap = np.asarray(prob.model.model_var_to_optimizer, dtype=np.int64)
            g.assert_terms_equal(quad, U.restate(prob.current("Q"), prob.xvar, 1, varmap))
            assert len(lin) == 0 and const == 0.0
    finally:
        prob.model.close()


def test_device_handoff_is_the_upper_triangle_of_the_pairs():
    """handoff="device" (the generic route): P's CSC pattern is the form's pairs by (column, row), its values the pairs' coefficients bit
    for bit (one term per pair: nothing is added), q is zero and r is 0.0"""
    prob = Problem("bare", handoff="device", optimizer=P.MockOptimizer(), extra=0)
    try:
        for it in range(2):
            if it:
                prob.new_values(77)
            P.solve(prob.model)
            assert prob.model.objective.mode == "canonical-sparse-form"
            qp = prob.model.device_qp.fetch()
            Q = prob.current("Q")
            n = prob.n
            pj, pk, sa, sb = U.tables(Q)
            coeff = U.coefficients(Q.data, (pj, pk, sa, sb), 1)
            order = np.lexsort((pj, pk))                                   # CSC: by column k, then row j
            values, row_idx, col_ptr = qp["P"]
            assert np.array_equal(row_idx, pj[order]) and np.array_equal(col_ptr, np.concatenate([[0], np.cumsum(np.bincount(pk, minlength=n))]))
            assert g.same_bits(values, coeff[order])
            assert np.all(qp["q"] == 0.0) and qp["r"] == 0.0
    finally:
        prob.model.close()


def test_literal_mode_and_host_csc_raise_at_initialize():
    for kw, what in (({"quadratic_mode": "literal"}, "quadratic_mode='literal'"), ({"handoff": "host_csc"}, "handoff='host_csc'")):
        prob = Problem("bare", **kw)
        try:
            with pytest.raises(_lib.ArgumentError, match=what):
                P.solve(prob.model)
        finally:
            prob.model.close()


# ---- 4. sums
CASES = [("weighted", "small, auto"), ("weighted", "graph, canonical"), ("qp", "small, auto"), ("qp", "graph, auto"), ("block", "small, auto"),
         ("block", "graph, canonical"), ("ridge", "small, auto"), ("ridge", "graph, auto"), ("two", "small, auto"), ("two", "graph, canonical"),
         ("part", "graph, auto"), ("part", "small, canonical")]


@pytest.mark.parametrize("kind,flavour", CASES, ids=["%s; %s" % c for c in CASES])
def test_sums_with_a_form_bit_for_bit_solve_after_solve(kind, flavour):
    kw, small = MODELS[flavour]
    prob = Problem(kind, **kw)
    try:
        nbytes = []
        for it in range(3):
            if it:
                prob.new_values(50 + it)
            quad, lin, const = prob.solved()
            assert prob.model.objective.mode == "canonical-sparse-sum" and prob.model._small == small
            varmap = np.asarray(prob.model.model_var_to_optimizer, dtype=np.int64)
            wq, wl, wc = U.sum_restate(prob.n, prob.xvar, varmap, prob.terms())
            g.assert_terms_equal(quad, wq)
            g.assert_terms_equal(lin, wl)
            assert g.same_bits([const], [wc])
            if kind in ("weighted", "two", "part"):
                assert len(lin) == 0
            nbytes.append(prob.model.device().bytes_allocated())
        assert len(set(nbytes)) == 1, "plan memory grew across solves: %r" % (nbytes,)
    finally:
        prob.model.close()


def test_a_dense_block_or_form_beside_raises_with_the_reason():
    for kind, kw in (("dense block beside", {}), ("dense block beside", {"quadratic_mode": "canonical", "use_graph": True}),
                     ("dense form beside", {}), ("dense form beside", {"quadratic_mode": "canonical", "use_graph": True})):
        prob = Problem(kind, **kw)
        try:
            with pytest.raises(_lib.ArgumentError, match="sparse Q has no literal form"):
                P.solve(prob.model)
        finally:
            prob.model.close()


# ---- 5. one solved model
def test_a_solved_qp_equals_its_dense_statement():
    """minimize 1/2 x'Qx + q'x subject to A x == b, n = 12, three equality rows, Q unsymmetric and sparse with a diagonal in [4, 5) and a
    few off-diagonal entries of at most 0.25 (Q + Q' is strictly diagonally dominant: strictly convex), through the KKT solve of
    tests/qp_solver.py; the same model with Q held as a dense Parameter.
    Bound 1e-9: by test_equals_the_dense_form_node_on_the_densified_matrix the two objectives hold EQUAL coefficients at the sparse pairs
    and the dense function's other coefficients are 0.0; q, A and b are the same host data.  The two KKT systems K z = rhs therefore hold
    equal numbers up to the last-place effects of the 0.5 * weights and of adding zeros, |dK| <= a few 2^-53 |K|, and the solutions differ
    by at most cond(K) * |dK| / |K| * |z|: with cond(K) < 1e3 (asserted) and |z| of order 1 that is below 1e-12, three orders inside 1e-9."""
    from qp_solver import DenseQPOptimizer
    rng = np.random.default_rng(12)
    n = 12
    M = np.triu(rng.random((n, n)) < 0.25, 1)
    r, c = np.nonzero(M | (rng.random((n, n)) < 0.1))
    off = r != c
    Q = U.from_entries(n, np.concatenate([r[off], np.arange(n)]), np.concatenate([c[off], np.arange(n)]),
                       np.concatenate([0.5 * SG.signed_values(rng, int(off.sum())), 4.0 + rng.random(n)]))
    q, A, b = SG.signed_values(rng, n), rng.standard_normal((3, n)), rng.standard_normal(3)
    sols = []
    for dense in (False, True):
        model = P.Model(DenseQPOptimizer(), quadratic_mode="canonical", use_graph=dense)
        try:
            x = [P.Variable(model) for _ in range(n)]
            Qp = P.Parameter((lambda: Q.toarray()) if dense else (lambda: Q), model)
            qp, Ap, bp = P.Parameter(lambda: q, model), P.Parameter(lambda: A, model), P.Parameter(lambda: b, model)
            P.objective(model, P.Minimize, 0.5 * (P.transpose(x) * Qp * x) + P.dot(qp, x))
            P.constraint(model, Ap * x == bp)
            P.solve(model)
            assert model.objective.mode == ("canonical-sum" if dense else "canonical-sparse-sum")
            sols.append(np.array([P.value(model, v) for v in x]))
        finally:
            model.close()
    K = np.block([[0.5 * (Q.toarray() + Q.toarray().T), A.T], [A, np.zeros((3, 3))]])
    assert np.linalg.cond(K) < 1e3
    assert np.max(np.abs(sols[0] - sols[1])) <= 1e-9
    np.testing.assert_allclose(A @ sols[0], b, atol=1e-9)
