"""-m gpu: weighted sums over sparse least-squares blocks (pmt_sparse_gram_sum_f64, csrc/sparse_gram_sum.hip; record mode
"canonical-sparse-sum").  Through the C ABI the combine alone, on synthetic block lists: guard words around every poisoned output, the
output bit for bit against the Python restatement of the contract (sparse_sum_util.restate, proven against the oracle on the CPU).
Through Model: dot(r, r) + lam*dot(x, x) and the other sums, small and beyond the small plan, solve after solve, against the restatement
bit for bit and the oracle within the derived bound (sparse_sum_util.bounds); both hand-offs; and the errors that stay."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sp = pytest.importorskip("scipy.sparse")

import gpu_util as g  # noqa: E402
import parametron_jl_amd as P  # noqa: E402
import sparse_gram_util as SG  # noqa: E402
import sparse_sum_util as U  # noqa: E402
from parametron_jl_amd import _lib  # noqa: E402
from sparse_sum_util import Term  # noqa: E402
from test_gpu_sparse_gram import POISON, Perm, check_bits, dev_bytes, make_vars  # noqa: E402

LT, QT = _lib.LT, _lib.QT
WG = _lib.PMT_SPARSE_SUM_WG_TERMS                  # output terms per workgroup (include/parametron_hip.h)
KIND = {"block": _lib.PMT_LSQ_BLOCK, "diag": _lib.PMT_LSQ_DIAG, "linear": _lib.PMT_LSQ_LINEAR, "constant": _lib.PMT_LSQ_CONSTANT}


def test_the_header_and_the_binding_agree_on_the_workgroup_count():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "parametron_hip.h")).read()
    assert int(re.search(r"#define PMT_SPARSE_SUM_WG_TERMS (\d+)", hdr).group(1)) == WG


# ---- through the C ABI: the combine alone, on synthetic block lists
def synthetic(rng, K, n, N, nlin):
    """A term list whose merged structure has exactly N quadratic pairs and nlin linear columns over n positions, and the blocks' lists:
    K blocks with random pair / column sets, a diagonal term over positions 3 and 17 — (3, 3) is also a block pair, (17, 17) is a pure-D
    pair —, a linear term over part of x whose first column no block has (linear-only), a diagonal term with v over two block columns
    (N >= 8), two constants.  Weights: host scales and device scalars, some negative.  N == 1: the pure-D pair alone; N == 0: no pair."""
    allp = [(j, k) for j in range(n) for k in range(j, n)]
    assert N <= len(allp) and nlin <= n
    lcols = sorted(rng.choice(n, nlin, replace=False).tolist())
    lin_only = lcols[0] if nlin else None
    dv = [c for c in lcols[1:3]] if (N >= 8 and nlin >= 3) else []
    forced = ({(3, 3), (17, 17)} if N >= 2 else ({(17, 17)} if N == 1 else set())) | {(c, c) for c in dv}
    rest = [p for p in allp if p not in forced]
    pick = [rest[i] for i in sorted(rng.choice(len(rest), N - len(forced), replace=False).tolist())] if N > len(forced) else []
    held = sorted(set(pick) | ({(3, 3)} if N >= 2 else set()))            # the pairs some block holds; (c, c) of dv and (17, 17) come from D alone
    member = {p: set(rng.choice(K, int(rng.integers(1, K + 1)), replace=False).tolist()) for p in held}
    lmember = {c: set(rng.choice(K, int(rng.integers(1, K + 1)), replace=False).tolist()) for c in lcols if c != lin_only and c not in dv[1:]}
    terms, blocks = [], []
    for b in range(K):
        pat = ([(j, k, None) for (j, k) in held if b in member[(j, k)]], [c for c in lcols if b in lmember.get(c, ())])
        w = [dict(scale=1.0), dict(scale=-0.75), dict(scale=2.0, weight=float(rng.random() - 0.5)), dict(weight=-1.5)][b % 4]
        terms.append(Term("block", pat=pat, **w))
        Q, L = np.zeros(len(pat[0]), dtype=QT), np.zeros(len(pat[1]), dtype=LT)
        Q["coeff"], Q["row"], Q["col"] = SG.signed_values(rng, len(Q)), -11, -12          # (the combine reads the coefficient words only)
        L["coeff"], L["var"] = SG.signed_values(rng, len(L)), -13
        blocks.append((Q, L, float(rng.random() - 0.5)))
        if b == 0 and N >= 1:
            terms.append(Term("diag", cols=[3, 17] if N >= 2 else [17], weight=float(rng.random() + 0.25), scale=-1.0 if K == 2 else 1.0))
    if dv:
        terms.append(Term("diag", cols=dv, v=SG.signed_values(rng, len(dv)), sign=-1, scale=0.5))
    if nlin:
        part = sorted({lin_only} | set(rng.choice(lcols, max(1, nlin // 2), replace=False).tolist()))
        terms.append(Term("linear", cols=part, v=SG.signed_values(rng, len(part)), weight=float(-rng.random())))
    terms += [Term("constant", scale=3.25), Term("constant", value=float(rng.random() - 0.5), scale=-1.0)]
    pairs, cols = U.structure(n, terms)
    assert len(pairs) == N and len(cols) == nlin, (len(pairs), len(cols))
    if N >= 2:
        assert (17, 17) in pairs and (17, 17) not in held
    if nlin:
        assert all(lin_only not in t.pat[1] for t in terms if t.kind == "block")
    return terms, blocks


def run_abi(n, xvar, varmap, terms, blocks, odd=False):
    """One call of pmt_sparse_gram_sum_f64 on the library's own merge of this term list.  Every output sits between guard words (`odd`:
    an odd number of them in front, so that the output's base is 8 mod 16) and starts out poisoned; returns (quad, lin, constant)."""
    g.lib()
    S = U.merge_tables(n, terms)
    keep = []

    def dev(a):
        t = dev_bytes(a)
        keep.append(t)
        return t.data_ptr()
    desc, k = [], 0
    for i, t in enumerate(terms):
        d = {"kind": KIND[t.kind], "scale": t.scale, "weight": dev(np.array([t.weight])) if t.weight is not None else None}
        if t.kind == "block":
            Q, L, cc = blocks[k]
            d.update(quad=dev(Q), lin=dev(L), constant=dev(np.array([cc])), quad_at=dev(S.quad_at[k]), lin_at=dev(S.lin_at[k]))
            k += 1
        elif t.kind in ("diag", "linear"):
            d.update(vec=dev(t.v) if t.v is not None else None, sign=t.sign if t.kind == "diag" and t.v is not None else 0,
                     pos=dev(S.term_pos[i]) if i in S.term_pos else None, nvec=len(t.positions(n)))
        elif t.value is not None:
            d["vec"] = dev(np.array([t.value]))
        desc.append(d)
    arr = _lib.sparse_lsq_terms(desc)
    dx, dvm = g.to_dev(np.asarray(xvar, dtype=np.int64)), g.to_dev(np.asarray(varmap, dtype=np.int64))
    G = 5 if odd else 4
    oq = torch.full((2 * G + 3 * S.nq,), POISON, dtype=torch.int64, device=g.DEV)
    ol = torch.full((2 * G + 2 * S.nlin,), POISON, dtype=torch.int64, device=g.DEV)
    oc = torch.full((2 * G + 1,), POISON, dtype=torch.int64, device=g.DEV)
    base = lambda t: C.c_void_p(t.data_ptr() + 8 * G)                     # noqa: E731
    assert (oq.data_ptr() + 8 * G) % 16 == (8 if odd else 0)
    vp = C.c_void_p
    g.call("pmt_sparse_gram_sum_f64", n, C.addressof(arr), len(desc), vp(dev(S.pair_j)), vp(dev(S.pair_k)), S.nq, vp(dev(S.lin_col)), S.nlin, g.ptr(dx),
           g.ptr(dvm), base(oq), base(ol), base(oc), g.stream())
    torch.cuda.synchronize()
    out = []
    for buf, words in ((oq, 3 * S.nq), (ol, 2 * S.nlin), (oc, 1)):
        h = buf.cpu().numpy()
        assert np.all(h[:G] == POISON) and np.all(h[G + words:] == POISON), "a guard word was overwritten"
        out.append(h[G:G + words].copy())
    return out[0].view(QT), out[1].view(LT), float(out[2].view(np.float64)[0])


# (K, n, output quadratic terms, output linear terms, output base 8 mod 16): the edges come from the header's per-workgroup count
ABI = [(1, 40, 0, 0, False), (2, 40, 1, 1, True), (1, 40, WG - 1, 17, False), (2, 40, WG, 40, True), (3, 40, WG + 1, 39, False),
       (8, 40, 3 * WG + 37, 40, True), (3, 40, 3 * WG + 37, 33, False), (2, 300, WG + 70, WG - 1, False), (3, 300, 2 * WG, WG, True),
       (8, 300, 40, WG + 1, False)]


@pytest.mark.parametrize("K,n,N,nlin,odd", ABI, ids=["K%d n%d nq%d nlin%d%s" % (c[0], c[1], c[2], c[3], " odd" if c[4] else "") for c in ABI])
def test_combine_bit_for_bit_at_the_c_abi(K, n, N, nlin, odd):
    rng = np.random.default_rng(1000 * K + N + nlin)
    terms, blocks = synthetic(rng, K, n, N, nlin)
    xvar, varmap = make_vars(rng, n)
    got = run_abi(n, xvar, varmap, terms, blocks, odd=odd)
    want = U.restate(n, xvar, varmap, terms, blocks=blocks)
    assert (len(got[0]), len(got[1])) == (N, nlin)
    check_bits(got, want)
    if N >= 2:                                       # the pure-D pair holds D alone: ((2*W_d)) of the one diagonal term that lists 17
        pairs, _ = U.structure(n, terms)
        dterm = [t for t in terms if t.kind == "diag" and t.v is None][0]
        assert got[0]["coeff"][pairs.index((17, 17))] == 2 * dterm.W


# ---- through Model
class Problem:
    """minimize a weighted sum over sparse blocks r_b = C_b*x - d_b (host-updated sparse Parameters of fixed patterns) and simple terms"""

    def __init__(self, kind, m=60, n=30, density=0.1, seed=1, optimizer=None, extra=2, dense=False, **kw):
        rng = np.random.default_rng(seed)
        self.kind, self.n = kind, n
        mask = rng.random((m, n)) < density
        mask[:, 4] = False                                                 # an empty column: its diagonal pair and linear term come from the other terms alone
        self.C1, self.C2 = SG.from_mask(mask, rng), SG.random_csc(rng, m // 2 + 7, n, 1.5 * density)
        self.part = np.array([1, 2, 5, 11, 12, n - 1])                    # u: a strictly increasing part of x
        self.st = st = {"C1": self.C1.data.copy(), "C2": self.C2.data.copy(), "d1": SG.signed_values(rng, m), "d2": SG.signed_values(rng, m // 2 + 7),
                        "lam": 0.25, "w1": 1.5, "w2": -0.625, "p": SG.signed_values(rng, n), "c": SG.signed_values(rng, n), "s": 0.75}
        self.model = model = P.Model(optimizer or Perm(), **kw)
        pre = [P.Variable(model) for _ in range(extra)]                    # x does not start at Variable 1
        x = [P.Variable(model) for _ in range(n)]
        self.xvar = np.arange(extra + 1, extra + n + 1, dtype=np.int64)
        self.nvars = len(pre) + n

        def sparse(key, Cs):
            def upd(Cm):
                Cm.data[:] = st[key]
            if dense:
                return P.Parameter(lambda: self.current(key).toarray(), model)
            return P.Parameter(upd, Cs.copy(), model)
        par = lambda key: P.Parameter(lambda: st[key], model)             # noqa: E731
        r1 = sparse("C1", self.C1) * x - par("d1")
        if kind == "ridge":
            expr = P.dot(r1, r1) + par("lam") * P.dot(x, x)
        elif kind == "two":
            r2 = sparse("C2", self.C2) * x + par("d2")
            expr = par("w1") * P.dot(r1, r1) + par("w2") * P.dot(r2, r2)
        elif kind == "mixed":
            p = par("p")
            expr = P.transpose(r1) * r1 + P.dot(x - p, x - p) + P.dot(par("c"), x) + par("s")
        elif kind == "part":
            u = [x[i] for i in self.part]
            expr = P.dot(r1, r1) - 0.5 * P.dot(u, u)
        elif kind == "scaled":
            expr = 2.0 * P.dot(r1, r1)
        elif kind == "shifted":
            expr = P.dot(r1, r1) + par("s")
        elif kind == "bare":
            expr = P.dot(r1, r1)
        elif kind == "dense beside sparse":
            A = P.Parameter(lambda: np.ones((5, n)), model)
            r2 = A * x
            expr = P.dot(r1, r1) + P.dot(r2, r2)
        P.objective(model, P.Minimize, expr)

    def current(self, key):
        Cs = (self.C1 if key == "C1" else self.C2).copy()
        Cs.data[:] = self.st[key]
        return Cs

    def new_values(self, seed):
        rng = np.random.default_rng(seed)
        st = self.st
        for k in ("C1", "C2", "d1", "d2", "p", "c"):
            st[k] = SG.signed_values(rng, len(st[k]))
        st["lam"], st["w1"], st["w2"], st["s"] = float(rng.uniform(0.1, 2)), float(rng.uniform(-2, 2)), float(rng.uniform(-2, 2)), float(rng.standard_normal())

    def terms(self):
        """the sum in plain data, in expression order, at the current values"""
        st = self.st
        b1 = dict(Cs=self.current("C1"), d=st["d1"], sign=-1)
        return {"ridge": lambda: [Term("block", **b1), Term("diag", weight=st["lam"])],
                "two": lambda: [Term("block", weight=st["w1"], **b1), Term("block", weight=st["w2"], Cs=self.current("C2"), d=st["d2"], sign=1)],
                "mixed": lambda: [Term("block", **b1), Term("diag", v=st["p"], sign=-1), Term("linear", v=st["c"]), Term("constant", value=st["s"])],
                "part": lambda: [Term("block", **b1), Term("diag", cols=self.part, scale=-0.5)],
                "scaled": lambda: [Term("block", scale=2.0, **b1)],
                "shifted": lambda: [Term("block", **b1), Term("constant", value=st["s"])]}[self.kind]()

    def solved(self):
        P.solve(self.model)
        f = self.model.objective.f
        return f.quadratic_terms.copy(), f.affine_terms.copy(), float(f.constant)


MODELS = {"small, auto": ({}, True), "graph, auto": ({"use_graph": True}, False), "graph, canonical": ({"quadratic_mode": "canonical", "use_graph": True}, False)}
CASES = [("ridge", "small, auto"), ("ridge", "graph, auto"), ("ridge", "graph, canonical"), ("two", "graph, auto"), ("two", "small, auto"),
         ("mixed", "graph, canonical"), ("mixed", "small, auto"), ("part", "graph, auto"), ("scaled", "small, auto"), ("scaled", "graph, auto")]


@pytest.mark.parametrize("kind,flavour", CASES, ids=["%s; %s" % c for c in CASES])
def test_model_against_restatement_and_oracle_solve_after_solve(kind, flavour):
    kw, small = MODELS[flavour]
    prob = Problem(kind, **kw)
    try:
        nbytes = []
        for it in range(3):
            if it:
                prob.new_values(50 + it)
            got = prob.solved()
            assert prob.model.objective.mode == "canonical-sparse-sum" and prob.model._small == small
            varmap = np.asarray(prob.model.model_var_to_optimizer, dtype=np.int64)
            assert np.array_equal(varmap, np.arange(prob.nvars, 0, -1) + 10)
            terms = prob.terms()
            check_bits(got, U.restate(prob.n, prob.xvar, varmap, terms))
            U.assert_close_to_oracle(*got, U.oracle_function(prob.n, prob.xvar, varmap, terms), *U.bounds(prob.n, terms))
            nbytes.append(prob.model.device().bytes_allocated())
        assert len(set(nbytes)) == 1, "plan memory grew across solves: %r" % (nbytes,)
    finally:
        prob.model.close()


@pytest.mark.parametrize("flavour", ["small, auto", "graph, auto"])
def test_a_sum_with_a_scalar_has_the_bare_node_s_bits(flavour):
    """dot(r, r) + s: W = 1 is exact, so the quadratic and linear terms are the bare node's bit for bit and the constant is the bare
    constant + s"""
    kw, _ = MODELS[flavour]
    shifted, bare = Problem("shifted", **kw), Problem("bare", **kw)
    try:
        for it in range(2):
            if it:
                shifted.new_values(61)
                bare.st.update(shifted.st)
            sq, sl, sc = shifted.solved()
            bq, bl, bc = bare.solved()
            assert shifted.model.objective.mode == "canonical-sparse-sum" and bare.model.objective.mode == "canonical-sparse"
            g.assert_terms_equal(sq, bq)
            g.assert_terms_equal(sl, bl)
            assert g.same_bits([sc], [bc + shifted.st["s"]])
    finally:
        shifted.model.close()
        bare.model.close()


def test_dense_twin_agrees_on_the_structural_pairs():
    """the same ridge with C held as a dense Parameter ("canonical-sum"): within the bound on the structural pairs; elsewhere the dense
    function holds 0.0 off the diagonal and the diagonal shift D = 2*lam alone on diagonal pairs the sparse pattern lacks"""
    sparse = Problem("ridge", use_graph=True)
    dense = Problem("ridge", use_graph=True, dense=True, quadratic_mode="canonical")
    try:
        sq, sl, sc = sparse.solved()
        dq, dl, dc = dense.solved()
        assert dense.model.objective.mode == "canonical-sum" and sparse.model.objective.mode == "canonical-sparse-sum"
        n = sparse.n
        assert len(dq) == n * (n + 1) // 2 and len(dl) == n
        terms = sparse.terms()
        bq, bl, bc = U.bounds(n, terms)
        pairs, cols = U.structure(n, terms)
        held = {(j, k) for j, k, _ in terms[0].pat[0]}
        assert all((j, j) in pairs for j in range(n)) and len(held) < len(pairs) < len(dq)          # the ridge fills the diagonal
        at = {(int(r), int(c)): k for k, (r, c) in enumerate(zip(dq["row"], dq["col"]))}
        hit = np.array([at[(int(r), int(c))] for r, c in zip(sq["row"], sq["col"])])
        assert len(set(hit.tolist())) == len(sq)
        assert np.all(np.abs(dq["coeff"][hit] - sq["coeff"]) <= bq)
        lone = np.array([p not in held for p in pairs])                                            # D alone, on both sides
        assert lone.any() and np.all(sq["coeff"][lone] == 2 * sparse.st["lam"]) and np.all(dq["coeff"][hit][lone] == 2 * sparse.st["lam"])
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


def test_device_handoff_is_the_upper_triangle_of_the_weighted_sum():
    """handoff="device": P is triu(2*(w1*C1'C1 + w2*C2'C2) + 2*lam*I) on the union pattern within the bound, q and r likewise"""
    rng = np.random.default_rng(4)
    m, n = 60, 30
    C1, C2 = SG.random_csc(rng, m, n, 0.1), SG.random_csc(rng, 37, n, 0.15)
    st = {"C1": C1.data.copy(), "C2": C2.data.copy(), "d1": SG.signed_values(rng, m), "d2": SG.signed_values(rng, 37), "w1": 1.5, "w2": 0.625, "lam": 0.25}
    model = P.Model(P.MockOptimizer(), handoff="device")
    try:
        x = [P.Variable(model) for _ in range(n)]
        xvar = np.arange(1, n + 1, dtype=np.int64)

        def sparse(key, Cs):
            def upd(Cm):
                Cm.data[:] = st[key]
            return P.Parameter(upd, Cs.copy(), model)
        par = lambda key: P.Parameter(lambda: st[key], model)             # noqa: E731
        r1, r2 = sparse("C1", C1) * x - par("d1"), sparse("C2", C2) * x - par("d2")
        P.objective(model, P.Minimize, par("w1") * P.dot(r1, r1) + par("w2") * P.dot(r2, r2) + par("lam") * P.dot(x, x))
        for it in range(2):
            if it:
                r = np.random.default_rng(78)
                for k in ("C1", "C2", "d1", "d2"):
                    st[k] = SG.signed_values(r, len(st[k]))
                st["w1"], st["w2"], st["lam"] = 0.75, 1.25, 0.5
            P.solve(model)
            assert model.objective.mode == "canonical-sparse-sum"
            qp = model.device_qp.fetch()
            A1, A2 = C1.copy(), C2.copy()
            A1.data[:], A2.data[:] = st["C1"], st["C2"]
            terms = [Term("block", weight=st["w1"], Cs=A1, d=st["d1"], sign=-1), Term("block", weight=st["w2"], Cs=A2, d=st["d2"], sign=-1),
                     Term("diag", weight=st["lam"])]
            pairs, cols = U.structure(n, terms)
            bq, bl, bc = U.bounds(n, terms)
            patt = sp.triu(abs(A1).T @ abs(A1) + abs(A2).T @ abs(A2) + sp.identity(n)).tocsc()
            patt.sort_indices()
            values, row_idx, col_ptr = qp["P"]
            assert np.array_equal(col_ptr, patt.indptr) and np.array_equal(row_idx, patt.indices)
            full = (2 * (st["w1"] * (A1.T @ A1) + st["w2"] * (A2.T @ A2))).toarray() + 2 * st["lam"] * np.eye(n)
            pcols = np.repeat(np.arange(n), np.diff(patt.indptr))
            bound = dict(zip(pairs, bq))
            tol = np.array([bound[(int(j), int(k))] for j, k in zip(patt.indices, pcols)])
            assert len(tol) == len(pairs) and np.all(np.abs(values - full[patt.indices, pcols]) <= tol)
            c1, c2 = 0.0 - st["d1"], 0.0 - st["d2"]
            q, qb = np.zeros(n), np.zeros(n)
            q[cols], qb[cols] = (2 * (st["w1"] * (A1.T @ c1) + st["w2"] * (A2.T @ c2)))[cols], bl
            assert np.all(np.abs(qp["q"] - q) <= qb)
            assert abs(qp["r"] - (st["w1"] * float(c1 @ c1) + st["w2"] * float(c2 @ c2))) <= bc
    finally:
        model.close()


# ---- what stays an error
def test_literal_mode_host_csc_and_a_dense_block_beside_raise_as_before():
    for kind, kw in (("ridge", {"quadratic_mode": "literal"}), ("ridge", {"handoff": "host_csc"}), ("dense beside sparse", {}),
                     ("dense beside sparse", {"quadratic_mode": "canonical", "use_graph": True})):
        prob = Problem(kind, **kw)
        try:
            with pytest.raises(_lib.ArgumentError, match="rows of equal length"):
                P.solve(prob.model)
        finally:
            prob.model.close()
