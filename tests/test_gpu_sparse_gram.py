"""-m gpu: the sparse least-squares objective dot(r, r), r = C*x (+|-) d with a sparse C (pmt_sparse_gram_f64, csrc/sparse_gram.hip).
Through the C ABI: guard words around every output, the output bit for bit against the Python restatement of the contract
(sparse_gram_util.restate, proven against the oracle on the CPU) and, on the small shapes, against the oracle's literal function within
the derived bound (sparse_gram_util.bounds).  Through Model: small and beyond the small plan, solve after solve, both hand-offs."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sp = pytest.importorskip("scipy.sparse")

import gpu_util as g  # noqa: E402
import parametron_jl_amd as P  # noqa: E402
import sparse_gram_util as U  # noqa: E402
from parametron_jl_amd import _lib  # noqa: E402

LT, QT = _lib.LT, _lib.QT
POISON = -7


def dev_bytes(a):
    """device copy of a host table of any dtype (never empty: a null table pointer is an error of its own)"""
    raw = np.frombuffer(np.ascontiguousarray(a).tobytes() + b"\0" * 8, dtype=np.uint8)
    return torch.from_numpy(raw.copy()).to(g.DEV)


def run_abi(Cs, xvar, d=None, sign=0, moi=1, varmap=None, cap=2048, odd=False):
    """One call of pmt_sparse_gram_f64 on the library's own tables for this pattern.  Every output sits between guard words (`odd`: an odd
    number of them in front, so that the output's base is 8 mod 16) and starts out poisoned; returns (quad, lin, constant)."""
    g.lib()
    T = U.tables(Cs, cap)
    m = Cs.shape[0]
    tabs = {k: dev_bytes(getattr(T, k)) for k in T.TABLES}
    nz = g.to_dev(Cs.data if Cs.nnz else np.zeros(1))
    dx = g.to_dev(np.asarray(xvar, dtype=np.int64) if len(xvar) else np.zeros(1, dtype=np.int64))
    dd = g.to_dev(np.asarray(d, dtype=np.float64)) if d is not None else None
    dvm = g.to_dev(np.asarray(varmap, dtype=np.int64)) if varmap is not None else None
    G = 5 if odd else 4
    oq = torch.full((2 * G + 3 * T.nq,), POISON, dtype=torch.int64, device=g.DEV)
    ol = torch.full((2 * G + 2 * T.nlin,), POISON, dtype=torch.int64, device=g.DEV)
    oc = torch.full((2 * G + 1,), POISON, dtype=torch.int64, device=g.DEV)
    base = lambda t: C.c_void_p(t.data_ptr() + 8 * G)                     # noqa: E731
    assert (oq.data_ptr() + 8 * G) % 16 == (8 if odd else 0)
    g.call("pmt_sparse_gram_f64", g.ptr(nz), *T.call_args(m, lambda k: g.ptr(tabs[k])), g.ptr(dx), g.ptr(dd), sign if d is not None else 0, moi,
           g.ptr(dvm), base(oq), base(ol), base(oc), g.stream())
    torch.cuda.synchronize()
    out = []
    for buf, words in ((oq, 3 * T.nq), (ol, 2 * T.nlin), (oc, 1)):
        h = buf.cpu().numpy()
        assert np.all(h[:G] == POISON) and np.all(h[G + words:] == POISON), "a guard word was overwritten"
        out.append(h[G:G + words].copy())
    return out[0].view(QT), out[1].view(LT), float(out[2].view(np.float64)[0]), T


def check_bits(got, want):
    g.assert_terms_equal(got[0], want[0])
    g.assert_terms_equal(got[1], want[1])
    assert g.same_bits([got[2]], [want[2]])


def make_vars(rng, n, extra=5):
    """a strictly increasing x among n + extra variables and a permuting, shifted index map"""
    xvar = np.sort(rng.choice(np.arange(1, n + extra + 1), n, replace=False)).astype(np.int64)
    varmap = (rng.permutation(n + extra) + 1 + 3).astype(np.int64)
    return xvar, varmap


# ---- through the C ABI: bit for bit against the restatement
def test_short_long_switch_bit_for_bit():
    """m = 1000, n = 40 at 2 %, two full columns (segments of 1000 products: the one-wave order, also for their linear terms) and columns
    of exactly 63, 64 and 65 rows (either side of the switch)"""
    rng = np.random.default_rng(11)
    m, n = 1000, 40
    mask = rng.random((m, n)) < 0.02
    mask[:, 3], mask[:, 17] = True, True
    for col, cnt in ((8, 63), (9, 64), (10, 65)):
        mask[:, col] = False
        mask[rng.choice(m, cnt, replace=False), col] = True
    Cs = U.from_mask(mask, rng)
    assert [int(np.diff(Cs.indptr)[c]) for c in (8, 9, 10)] == [63, 64, 65]
    xvar, varmap = make_vars(rng, n)
    d = U.signed_values(rng, m)
    pat = U.pattern(Cs)
    lens = sorted(len(p) for _, _, p in pat[0])
    assert {63, 64, 65, 1000} <= set(lens) and lens[0] < 10
    for sign, moi in ((-1, 1), (1, 0)):
        got = run_abi(Cs, xvar, d, sign, moi, varmap if moi else None)
        T = got[3]
        assert T.nlong >= 5 and T.nruns >= 1 and T.nlin_long == 4 and T.nlin_runs >= 1
        check_bits(got, U.restate(Cs, xvar, d, sign, moi, varmap, pat))


def test_many_workgroups_bit_for_bit_and_independent_of_the_cut():
    """m = 20000, n = 5000, 4 per row banded: cut at 508 products it is 395 workgroup runs, 263 of them filled exactly to the cap (their
    last segment ends on the run boundary), the last one partial; the same call cut at 2048 writes the same bits"""
    rng = np.random.default_rng(12)
    m, n = 20000, 5000
    Cs = U.banded(rng, m, n, 4)
    xvar, varmap = make_vars(rng, n, extra=3)
    d = U.signed_values(rng, m)
    want = U.restate(Cs, xvar, d, -1, 1, varmap)
    got = run_abi(Cs, xvar, d, -1, 1, varmap, cap=508)
    T = got[3]
    per_run = T.seg_ptr[T.runs[1::2]] - T.seg_ptr[T.runs[0::2]]
    assert T.nruns == 395 and T.nlong == 0 and int(np.count_nonzero(per_run == 508)) == 263 and 0 < per_run[-1] < 508 and per_run.max() == 508
    assert T.nlin_runs == 162 and T.nlin_long == 0                       # 16 entries per column: 31 columns per linear run
    check_bits(got, want)
    wide = run_abi(Cs, xvar, d, -1, 1, varmap, cap=2048)
    assert wide[3].nruns < 120
    check_bits(wide, want)


# ---- through the C ABI: the restatement bit for bit AND the oracle within the bound
def _by_hand():
    """7 x 5: column 0 full, column 3 empty, row 4 empty, a 2 x 2 block, a lone entry"""
    dense = np.zeros((7, 5))
    dense[:, 0] = [0.5, -0.25, 0.125, 0.375, 0.0, -0.5, 0.25]
    dense[4, 0] = 0.0
    dense[0, 1], dense[1, 1], dense[0, 2], dense[1, 2] = 0.25, -0.375, -0.125, 0.5
    dense[6, 4] = -0.4375
    Cs = sp.csc_matrix(dense)
    Cs.sort_indices()
    return Cs


def _one_entry():
    return sp.csc_matrix((np.array([-0.3]), (np.array([2]), np.array([1]))), shape=(4, 3))


SMALL = {"7x5 by hand": _by_hand, "300x200 at 3 %": lambda: U.random_csc(np.random.default_rng(21), 300, 200, 0.03),
         "no entry": lambda: sp.csc_matrix((6, 4)), "one entry": _one_entry}
VARIANTS = [("moi, x - d", -1, 1, False), ("moi, x + d", 1, 1, False), ("moi, no d", 0, 1, False), ("native, x - d", -1, 0, False),
            ("native, no d", 0, 0, False), ("moi, x - d, base 8 mod 16", -1, 1, True), ("native, x + d, base 8 mod 16", 1, 0, True)]


@pytest.fixture(scope="module")
def small_cases():
    """per shape: the matrix, x, the index map, d, the brute-force pattern, and the oracle's functions for the three residuals — computed once"""
    out = {}
    for k, (name, make) in enumerate(SMALL.items()):
        rng = np.random.default_rng(30 + k)
        Cs = make()
        m, n = Cs.shape
        xvar, varmap = make_vars(rng, n)
        d = U.signed_values(rng, m)
        pat = U.pattern(Cs)
        oracle = {sign: U.oracle_function(Cs, xvar, d if sign else None, sign, varmap) for sign in (-1, 0, 1)}
        bound = {sign: U.bounds(Cs, d if sign else None, sign, pat) for sign in (-1, 0, 1)}
        out[name] = (Cs, xvar, varmap, d, pat, oracle, bound)
    return out


@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize("shape", list(SMALL))
def test_small_shapes_against_restatement_and_oracle(small_cases, shape, variant):
    _, sign, moi, odd = variant
    Cs, xvar, varmap, d, pat, oracle, bound = small_cases[shape]
    dd = d if sign else None
    quad, lin, const, T = run_abi(Cs, xvar, dd, sign, moi, varmap if moi else None, odd=odd)
    assert (len(quad), len(lin)) == (len(pat[0]), len(pat[1]))
    check_bits((quad, lin, const), U.restate(Cs, xvar, dd, sign, moi, varmap, pat))
    if shape == "no entry":
        assert len(quad) == 0 and len(lin) == 0
    if not sign:
        assert np.all(lin["coeff"] == 0.0) and const == 0.0                  # the terms exist, with zero coefficients
    if moi:
        U.assert_close_to_oracle(quad, lin, const, oracle[sign], *bound[sign])
    else:
        # the native form against the oracle's MOI function: native indices, the diagonal coefficient not doubled
        at, qt, oc = oracle[sign]
        inv = {int(varmap[v - 1]): int(v) for v in xvar}
        assert [inv[int(v)] for v in qt["row"]] == quad["row"].tolist() and [inv[int(v)] for v in qt["col"]] == quad["col"].tolist()
        assert [inv[int(v)] for v in at["var"]] == lin["var"].tolist()
        dbl = np.where(quad["row"] == quad["col"], 2.0, 1.0)
        assert np.all(np.abs(dbl * quad["coeff"] - qt["coeff"]) <= bound[sign][0])
        assert np.all(np.abs(lin["coeff"] - at["coeff"]) <= bound[sign][1]) and abs(const - oc) <= bound[sign][2]


# ---- through Model
class Perm(P.MockOptimizer):
    def copy_to(self, backend):
        out = super().copy_to(backend)
        out["variables"] = out["variables"][::-1].copy() + 10
        return out


class Problem:
    """minimize dot(C*x - d, C*x - d) with a host-updated sparse Parameter C (fixed pattern) and a host-updated d"""

    def __init__(self, m=60, n=30, density=0.1, seed=1, form="dot", dense=False, optimizer=None, extra=2, **kw):
        rng = np.random.default_rng(seed)
        self.Cs = Cs = U.random_csc(rng, m, n, density)
        self.st = st = {"data": Cs.data.copy(), "d": U.signed_values(rng, m)}
        self.model = model = P.Model(optimizer or Perm(), **kw)
        pre = [P.Variable(model) for _ in range(extra)]                    # x does not start at Variable 1
        x = [P.Variable(model) for _ in range(n)]
        self.xvar = np.arange(extra + 1, extra + n + 1, dtype=np.int64)
        self.nvars = len(pre) + n

        def upd(Cm):
            Cm.data[:] = st["data"]
        if dense:
            Cp = P.Parameter(lambda: self.current().toarray(), model)
        else:
            Cp = P.Parameter(upd, Cs.copy(), model)
        dp = P.Parameter(lambda: st["d"], model)
        r = Cp * x - dp
        P.objective(model, P.Minimize, P.dot(r, r) if form == "dot" else P.transpose(r) * r)

    def current(self):
        Cs = self.Cs.copy()
        Cs.data[:] = self.st["data"]
        return Cs

    def new_values(self, seed):
        rng = np.random.default_rng(seed)
        self.st["data"], self.st["d"] = U.signed_values(rng, self.Cs.nnz), U.signed_values(rng, self.Cs.shape[0])

    def solved(self):
        P.solve(self.model)
        f = self.model.objective.f
        return f.quadratic_terms.copy(), f.affine_terms.copy(), float(f.constant)


@pytest.mark.parametrize("kw,small", [({}, True), ({"use_graph": True}, False), ({"quadratic_mode": "canonical", "use_graph": True}, False)],
                         ids=["small, auto", "graph, auto", "graph, canonical"])
def test_model_against_the_oracle_solve_after_solve(kw, small):
    prob = Problem(**kw)
    twin = Problem(form="transpose", **kw)                                  # transpose(r) * r: the same node
    try:
        nbytes = []
        for it in range(3):
            if it:
                prob.new_values(50 + it)
                twin.st.update(prob.st)
            got = prob.solved()
            assert prob.model.objective.mode == "canonical-sparse" and prob.model._small == small
            varmap = np.asarray(prob.model.model_var_to_optimizer, dtype=np.int64)
            assert np.array_equal(varmap, np.arange(prob.nvars, 0, -1) + 10)
            Cs, d = prob.current(), prob.st["d"]
            check_bits(got, U.restate(Cs, prob.xvar, d, -1, 1, varmap))
            U.assert_close_to_oracle(*got, U.oracle_function(Cs, prob.xvar, d, -1, varmap), *U.bounds(Cs, d, -1))
            check_bits(twin.solved(), got)
            assert twin.model.objective.mode == "canonical-sparse"
            nbytes.append(prob.model.device().bytes_allocated())
        assert len(set(nbytes)) == 1, "plan memory grew across solves: %r" % (nbytes,)
    finally:
        prob.model.close()
        twin.model.close()


def test_dense_parameter_agrees_on_the_structural_pairs_and_is_zero_elsewhere():
    sparse = Problem(use_graph=True)
    dense = Problem(use_graph=True, dense=True, quadratic_mode="canonical")
    try:
        sq, sl, sc = sparse.solved()
        dq, dl, dc = dense.solved()
        assert dense.model.objective.mode == "canonical" and sparse.model.objective.mode == "canonical-sparse"
        n = sparse.Cs.shape[1]
        assert len(dq) == n * (n + 1) // 2 and len(dl) == n
        Cs, d = sparse.current(), sparse.st["d"]
        bq, bl, bc = U.bounds(Cs, d, -1)
        at = {(int(r), int(c)): k for k, (r, c) in enumerate(zip(dq["row"], dq["col"]))}
        hit = np.array([at[(int(r), int(c))] for r, c in zip(sq["row"], sq["col"])])
        assert len(set(hit.tolist())) == len(sq)
        assert np.all(np.abs(dq["coeff"][hit] - sq["coeff"]) <= bq)
        rest = np.ones(len(dq), dtype=bool)
        rest[hit] = False
        assert rest.any() and np.all(dq["coeff"][rest] == 0.0)
        lat = {int(v): k for k, v in enumerate(dl["var"])}
        lhit = np.array([lat[int(v)] for v in sl["var"]])
        assert np.all(np.abs(dl["coeff"][lhit] - sl["coeff"]) <= bl)
        lrest = np.ones(len(dl), dtype=bool)
        lrest[lhit] = False
        assert np.all(dl["coeff"][lrest] == 0.0)
        assert abs(dc - sc) <= bc
    finally:
        sparse.model.close()
        dense.model.close()


def test_device_handoff_is_the_upper_triangle_of_2_CtC():
    """handoff="device": P's CSC pattern and values are scipy.sparse.triu(2 * C' * C) within the bound, q is 2 * C' * c"""
    prob = Problem(handoff="device", optimizer=P.MockOptimizer(), extra=0)
    try:
        for it in range(2):
            if it:
                prob.new_values(77)
            P.solve(prob.model)
            assert prob.model.objective.mode == "canonical-sparse"
            qp = prob.model.device_qp.fetch()
            Cs, d = prob.current(), prob.st["d"]
            n = Cs.shape[1]
            A = abs(Cs)
            patt = sp.triu(A.T @ A).tocsc()
            patt.sort_indices()
            values, row_idx, col_ptr = qp["P"]
            assert np.array_equal(col_ptr, patt.indptr) and np.array_equal(row_idx, patt.indices)
            full = (2 * (Cs.T @ Cs)).toarray()
            cols = np.repeat(np.arange(n), np.diff(patt.indptr))
            pairs, lin_col = U.pattern(Cs)
            bq, bl, bc = U.bounds(Cs, d, -1, (pairs, lin_col))
            bound = {(j, k): b for (j, k, _), b in zip(pairs, bq)}
            tol = np.array([bound[(int(j), int(k))] for j, k in zip(patt.indices, cols)])
            assert np.all(np.abs(values - full[patt.indices, cols]) <= tol)
            c = 0.0 - d
            q = np.zeros(n)
            qb = np.zeros(n)
            q[lin_col], qb[lin_col] = (2 * (Cs.T @ c))[lin_col], bl
            assert np.all(np.abs(qp["q"] - q) <= qb)
            assert abs(qp["r"] - float(c @ c)) <= bc
    finally:
        prob.model.close()


def test_literal_mode_and_host_csc_raise_at_initialize():
    for kw, what in (({"quadratic_mode": "literal"}, "quadratic_mode='literal'"), ({"handoff": "host_csc"}, "handoff='host_csc'")):
        prob = Problem(**kw)
        try:
            with pytest.raises(_lib.ArgumentError, match=what):
                P.solve(prob.model)
        finally:
            prob.model.close()


def test_other_ragged_dots_raise_as_before():
    """a dot of two DIFFERENT sparse residuals and the node's literal value have no form"""
    prob = Problem()
    try:
        model = prob.model
        x = [P.Variable(model) for _ in range(prob.Cs.shape[1])]
        C1, C2 = P.Parameter(lambda Cm: None, prob.Cs.copy(), model), P.Parameter(lambda Cm: None, prob.Cs.copy(), model)
        with pytest.raises(_lib.ArgumentError, match="rows of equal length"):
            P.dot(C1 * x, C2 * x)
        r = C1 * x
        node = P.dot(r, r)
        with pytest.raises(_lib.ArgumentError, match="rows of equal length"):
            node()
    finally:
        prob.model.close()
