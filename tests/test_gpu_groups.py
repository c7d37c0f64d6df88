"""-m gpu: canonical objectives that are sums over disjoint Variable vectors (mode "canonical-groups"; csrc/groups.hip).

1. pmt_quad_groups_gather_f64 alone, bit for bit against a restatement by plain loops: random source words, a poisoned margin round the
   destination, every parity of source and destination segments.
2. The model path, word for word: the quadratic and linear terms are the (row, col) merge of what the SAME groups give as objectives of
   models of their own (modes "canonical-form" / "canonical-sum"), the constant is ((c_1 + c_2) + ..) in group order.  A bare form alone
   has no linear terms ("canonical-form"); in a sum it has n zero ones (include/parametron_hip.h: out_lin[j] = (0.0, vm[x_j])), so its
   part of the expected linear terms is (+0.0, varmap[x_j]).  A group of one bare block dot(r, r) is the header's sum of one block with
   weight 1, so its own model is 1.0 * dot(r, r) ("canonical-sum"): the bare objective ("canonical") has its terms delivered while they
   are computed, and a delivered call is never the tiny node (gram.hip: gram_form) — at 40 x 8 its sums run in another order.
3. Against the generic path (quadratic_mode="literal" + canonicalize(expr): the literal expansion, a sort, a segment sum): indices equal,
   coefficients within 1e-12 relative.  The data of this part are positive (A, B, b, d, c, the weights) so that no coefficient is a
   cancelling sum and "relative" needs no magnitude term; a form's coefficients Q[j,k] + Q[k,j] are exact in both paths.
4. Re-evaluation with changed Parameters, constant plan memory, graph replay."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import parametron_jl_amd as P  # noqa: E402
from parametron_jl_amd import _lib  # noqa: E402

DEV = "cuda:0"
GUARD = 16


def dptr(t, word=0):
    return C.c_void_p(t.data_ptr() + 8 * word)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------ 1. the gather entry alone
SIZES = [(1, 2), (3, 5, 4), (63, 66), (130, 1, 64), tuple(range(1, 9))]
ORDERS = ["ordered", "alternating", "random"]


def assign(sizes, order, seed=0):
    """the groups' variable sets over 1 .. sum(sizes)"""
    left = list(sizes)
    if order == "ordered":
        owner = [g for g, k in enumerate(sizes) for _ in range(k)]
    elif order == "alternating":
        owner = []
        while any(left):
            for g in range(len(sizes)):
                if left[g]:
                    owner.append(g)
                    left[g] -= 1
    else:
        owner = list(np.random.default_rng(seed).permutation([g for g, k in enumerate(sizes) for _ in range(k)]))
    owner = np.asarray(owner)
    return [np.flatnonzero(owner == g) + 1 for g in range(len(sizes))]


def restate_gather(sets, src_q, src_l):
    """(quadratic words, linear words, [(source term, destination term) of every row]) by plain loops over z"""
    n = [len(s) for s in sets]
    base = np.concatenate([[0], np.cumsum([k * (k + 1) // 2 for k in n])])
    lbase = np.concatenate([[0], np.cumsum(n)])
    where = {int(v): (g, j) for g, s in enumerate(sets) for j, v in enumerate(s)}
    q, lin, offs, dst = [], [], [], 0
    for v in sorted(where):
        g, j = where[v]
        s = base[g] + j * n[g] - j * (j - 1) // 2
        q.append(src_q[3 * s:3 * (s + n[g] - j)])
        lin.append(src_l[2 * (lbase[g] + j):2 * (lbase[g] + j) + 2])
        offs.append((int(s), dst))
        dst += n[g] - j
    return np.concatenate(q), np.concatenate(lin), offs


@pytest.mark.parametrize("shift", [0, 1], ids=["dst16", "dst8"])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: "x".join(map(str, s)))
def test_gather_entry(sizes, order, shift):
    sets = assign(sizes, order, seed=sum(sizes))
    lay = _lib.GroupsLayout(sets)
    rng = np.random.default_rng(len(sizes) * 1000 + sum(sizes))
    src_q = rng.integers(-2 ** 62, 2 ** 62, size=3 * lay.nterms, dtype=np.int64)
    src_l = rng.integers(-2 ** 62, 2 ** 62, size=2 * lay.nlin, dtype=np.int64)
    want_q, want_l, offs = restate_gather(sets, src_q, src_l)
    assert len(want_q) == 3 * lay.nterms and len(want_l) == 2 * lay.nlin
    # `shift`: the destination starts at an address 8 mod 16 (a leading single word)
    dq_src, dl_src = torch.from_numpy(src_q).to(DEV), torch.from_numpy(src_l).to(DEV)
    tabs = [torch.from_numpy(np.ascontiguousarray(t)).to(DEV) for t in (lay.row_src, lay.row_dst, lay.lin_src)]
    oq = torch.full((GUARD + shift + 3 * lay.nterms + GUARD,), -7, dtype=torch.int64, device=DEV)
    ol = torch.full((GUARD + 2 * lay.nlin + GUARD,), -7, dtype=torch.int64, device=DEV)
    assert oq.data_ptr() % 16 == 0
    _lib.call("pmt_quad_groups_gather_f64", dptr(dq_src), dptr(tabs[0]), dptr(tabs[1]), lay.nlin, lay.nterms, dptr(dl_src), dptr(tabs[2]), lay.nlin,
              dptr(oq, GUARD + shift), dptr(ol, GUARD), stream())
    torch.cuda.synchronize()
    hq, hl = oq.cpu().numpy(), ol.cpu().numpy()
    lo = GUARD + shift
    assert np.all(hq[:lo] == -7) and np.all(hq[lo + 3 * lay.nterms:] == -7), "the margin round the quadratic terms was written"
    assert np.all(hl[:GUARD] == -7) and np.all(hl[GUARD + 2 * lay.nlin:] == -7), "the margin round the linear terms was written"
    assert np.array_equal(hq[lo:lo + 3 * lay.nterms], want_q)
    assert np.array_equal(hl[GUARD:GUARD + 2 * lay.nlin], want_l)


def test_gather_cases_cover_every_parity():
    """(source, destination) term offsets odd / even in all four combinations over the cases above — host arithmetic over the same sets"""
    seen = set()
    for sizes in SIZES:
        for order in ORDERS:
            sets = assign(sizes, order, seed=sum(sizes))
            lay = _lib.GroupsLayout(sets)
            zero = np.zeros(3 * lay.nterms, dtype=np.int64)
            offs = restate_gather(sets, zero, np.zeros(2 * lay.nlin, dtype=np.int64))[2]
            for shift in (0, 1):
                seen.update((s % 2, (d + shift) % 2) for s, d in offs)
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_constant_entry():
    c = np.array([0.1, 0.2, 0.3, 1e-17, -0.6, 7.0, 1e300, -1e300])
    for g in range(1, 9):
        d = torch.from_numpy(c).to(DEV)
        out = torch.full((3,), float("nan"), dtype=torch.float64, device=DEV)
        _lib.call("pmt_quad_groups_constant_f64", dptr(d), g, dptr(out, 1), stream())
        torch.cuda.synchronize()
        want = c[0]
        for v in c[1:g]:
            want = want + v
        h = out.cpu().numpy()
        assert h[1:2].view(np.int64)[0] == np.array([want]).view(np.int64)[0] and np.isnan(h[0]) and np.isnan(h[2])


# ------------------------------------------------------------------ 2 .. 4. the model path
class Perm(P.MockOptimizer):
    def copy_to(self, backend):
        out = super().copy_to(backend)
        out["variables"] = out["variables"][::-1].copy() + 10
        return out


def values(kind, shape, seed, positive):
    rng = np.random.default_rng(seed)
    mat = (lambda r, c: rng.random((r, c)) + 0.1) if positive else (lambda r, c: rng.random((r, c)) - 0.5)
    st = {"lam": 0.75, "s": 1.25, "w": 0.5}
    if kind == "forms":
        nx, nu = shape
        st.update(Q=rng.standard_normal((nx, nx)), R=rng.standard_normal((nu, nu)))
    elif kind == "lsq2":
        (r1, nx), (r2, nu) = shape
        st.update(A=mat(r1, nx), b=rng.random(r1) + 0.1, B=mat(r2, nu), d=rng.random(r2) + 0.1)
    else:
        (r1, nx), nu = shape
        st.update(A=mat(r1, nx), b=rng.random(r1) + 0.1, R=rng.standard_normal((nu, nu)), c=rng.random(nu) + 0.1)
    return st, nx, nu


def group_exprs(kind, m, x, u, st):
    """the objective's groups as expressions of their own, in group order (constants with the first)"""
    par = lambda k: P.Parameter(lambda: st[k], m)          # noqa: E731
    if kind == "forms":
        return [P.transpose(x) * par("Q") * x, P.transpose(u) * par("R") * u]
    if kind == "lsq2":
        r1, r2 = par("A") * x - par("b"), par("B") * u - par("d")
        return [1.0 * P.dot(r1, r1), st["w"] * P.dot(r2, r2)]  # (a group of one bare block is the sum of one term with weight 1)
    r = par("A") * x - par("b")
    return [P.dot(r, r) + par("lam") * P.dot(x, x) + st["s"], P.transpose(u) * par("R") * u + P.dot(par("c"), u)]


def whole_expr(kind, m, x, u, st):
    """the objective as a user writes it: group 1's constant stands at the end of the third objective"""
    par = lambda k: P.Parameter(lambda: st[k], m)          # noqa: E731
    if kind == "forms":
        g = group_exprs(kind, m, x, u, st)
        return g[0] + g[1]
    if kind == "lsq2":
        r1, r2 = par("A") * x - par("b"), par("B") * u - par("d")
        return P.dot(r1, r1) + st["w"] * P.dot(r2, r2)
    r = par("A") * x - par("b")
    return P.dot(r, r) + par("lam") * P.dot(x, x) + P.transpose(u) * par("R") * u + P.dot(par("c"), u) + st["s"]


def build(kind, st, nx, nu, order, which, use_graph=False, permute=False, generic=False):
    """which: None = the whole objective, g = group g alone — over the same Variables created in the same order"""
    m = P.Model(Perm() if permute else P.MockOptimizer(), quadratic_mode="literal" if generic else "canonical", use_graph=use_graph)
    m.SMALL_MODEL_ELEMENTS = 0                               # beyond the small plan at sizes that keep the test fast
    x, u = [], []
    if order == "interleaved":
        for i in range(max(nx, nu)):
            if i < nx:
                x.append(P.Variable(m))
            if i < nu:
                u.append(P.Variable(m))
    else:
        for name in order:
            if name == "x":
                x = [P.Variable(m) for _ in range(nx)]
            else:
                u = [P.Variable(m) for _ in range(nu)]
    expr = whole_expr(kind, m, x, u, st) if which is None else group_exprs(kind, m, x, u, st)[which]
    P.objective(m, P.Minimize, expr.canonicalize() if generic else expr)
    return m, np.array([v.index for v in x], dtype=np.int64), np.array([v.index for v in u], dtype=np.int64)


def solved(m):
    P.solve(m)
    f = m.objective.f
    return f.quadratic_terms.copy(), f.affine_terms.copy(), float(f.constant)


def merged(parts, sets, varmap):
    """the (row, col) merge over model variables of the groups' own functions; a group without linear terms gives (+0.0, varmap[x_j])"""
    inv = np.zeros(int(np.max(varmap)) + 1, dtype=np.int64)
    inv[np.asarray(varmap)] = np.arange(1, len(varmap) + 1)
    back = lambda o: inv[o]                                # noqa: E731
    q = np.concatenate([p[0] for p in parts])
    lins = []
    for (pq, pl, pc), s in zip(parts, sets):
        if len(pl) == 0:
            pl = np.zeros(len(s), dtype=_lib.LT)
            pl["var"] = np.asarray(varmap)[s - 1]
        lins.append(pl)
    lin = np.concatenate(lins)
    q = q[np.lexsort((back(q["col"]), back(q["row"])))]
    lin = lin[np.argsort(back(lin["var"]), kind="stable")]
    const = parts[0][2]
    for p in parts[1:]:
        const = const + p[2]
    return q, lin, const


def words(a):
    return np.ascontiguousarray(a).view(np.int64)


def assert_same_words(got, want, what):
    g, w = words(got), words(want)
    assert g.shape == w.shape, "%s: %d words, expected %d" % (what, len(g), len(w))
    bad = np.flatnonzero(g != w)
    assert len(bad) == 0, "%s: %d of %d words differ, first at word %d (term %d): got %r, expected %r" % (
        what, len(bad), len(g), bad[0], bad[0] // (got.dtype.itemsize // 8), got[bad[0] // (got.dtype.itemsize // 8)], want[bad[0] // (got.dtype.itemsize // 8)])


def flat(shape):
    return [int(v) for part in shape for v in (part if isinstance(part, tuple) else (part,))]


CASES = [("forms", (65, 130), "xu"), ("forms", (65, 130), "interleaved"),
         ("lsq2", ((40, 8), (300, 70)), "ux"), ("lsq2", ((40, 8), (300, 70)), "interleaved"),
         ("lsq2", ((500, 100), (300, 300)), "xu"), ("lsq2", ((500, 100), (300, 300)), "interleaved"),
         ("qp", ((300, 70), 130), "xu"), ("qp", ((300, 70), 130), "interleaved")]
IDS = ["%s-%s-%s" % (k, "_".join(map(str, flat(s))), o) for k, s, o in CASES]
STANDALONE = {"forms": ["canonical-form", "canonical-form"], "lsq2": ["canonical-sum", "canonical-sum"], "qp": ["canonical-sum", "canonical-sum"]}


def perturb(st, seed):
    rng = np.random.default_rng(seed)
    for k, v in st.items():
        if isinstance(v, np.ndarray):
            st[k] = rng.standard_normal(v.shape) if k in ("Q", "R") else rng.random(v.shape) - 0.5
    st["lam"] = float(rng.uniform(0.1, 2))


@pytest.mark.parametrize("kind,shape,order", CASES, ids=IDS)
def test_model_words_equal_the_groups_own_models(kind, shape, order):
    st, nx, nu = values(kind, shape, seed=sum(flat(shape)), positive=False)
    m, xv, uv = build(kind, st, nx, nu, order, None)
    parts_m = [build(kind, st, nx, nu, order, g)[0] for g in range(2)]
    try:
        nbytes = []
        for it in range(4):
            if it:
                perturb(st, 77 + it)                         # Q / A, b and the weight Parameter change between two solve!s
            gq, gl, gc = solved(m)
            obj = m.objective
            assert obj.mode == "canonical-groups" and not m._small
            assert obj.groups_ordered == (order != "interleaved")
            parts = [solved(p) for p in parts_m]
            assert [p.objective.mode for p in parts_m] == STANDALONE[kind]          # the paths the groups take alone
            varmap = np.asarray(m.model_var_to_optimizer, dtype=np.int64)
            wq, wl, wc = merged(parts, [xv, uv], varmap)
            assert len(gq) == nx * (nx + 1) // 2 + nu * (nu + 1) // 2 and len(gl) == nx + nu
            assert_same_words(gq, wq, "quadratic terms against the groups' own")
            assert_same_words(gl, wl, "linear terms against the groups' own")
            assert words(np.array([gc]))[0] == words(np.array([wc]))[0], "constant is not ((c_1 + c_2) + ..)"
            # rows in increasing model variable, the columns of the row's own group in increasing order
            z = np.sort(np.concatenate([xv, uv]))
            assert np.array_equal(gl["var"], varmap[z - 1])
            nbytes.append(m.device().bytes_allocated())
        assert len(set(nbytes)) == 1, "plan memory grew across updates: %r" % (nbytes,)
    finally:
        m.close()
        for p in parts_m:
            p.close()


def test_an_ordered_case_starts_a_group_at_an_odd_term_offset():
    """host arithmetic: which slices of the ordered cases above start at an address 8 mod 16"""
    odd = []
    for kind, shape, order in CASES:
        if order == "interleaved":
            continue
        _, nx, nu = values(kind, shape, 0, False)
        first = nx if order == "xu" else nu
        odd.append((first * (first + 1) // 2) % 2 == 1)
    assert any(odd)


@pytest.mark.parametrize("order", ["xu", "interleaved"])
@pytest.mark.parametrize("kind,shape", [("forms", (65, 130)), ("qp", ((300, 70), 130))], ids=["forms", "qp"])
def test_graph_replay_and_permuted_varmap_give_the_same_words(kind, shape, order):
    st, nx, nu = values(kind, shape, seed=5, positive=False)
    a, xv, uv = build(kind, st, nx, nu, order, None)
    g, _, _ = build(kind, st, nx, nu, order, None, use_graph=True)
    p, _, _ = build(kind, st, nx, nu, order, None, permute=True)
    try:
        for it in range(2):
            if it:
                perturb(st, 9)
            ra, rg, rp = solved(a), solved(g), solved(p)
            assert g.objective.mode == p.objective.mode == "canonical-groups"
            for x, y in zip(ra, rg):
                assert np.array_equal(words(np.atleast_1d(x)), words(np.atleast_1d(y)))
            # the permuted optimizer: the same terms in the same places, indices through the varmap
            vm = np.asarray(p.model_var_to_optimizer, dtype=np.int64)
            assert np.array_equal(vm, np.arange(nx + nu, 0, -1) + 10)
            assert np.array_equal(words(rp[0]["coeff"]), words(ra[0]["coeff"])) and np.array_equal(words(rp[1]["coeff"]), words(ra[1]["coeff"]))
            assert np.array_equal(rp[0]["row"], vm[ra[0]["row"] - 1]) and np.array_equal(rp[0]["col"], vm[ra[0]["col"] - 1])
            assert np.array_equal(rp[1]["var"], vm[ra[1]["var"] - 1]) and rp[2] == ra[2]
    finally:
        for m in (a, g, p):
            m.close()


GENERIC = [("forms", (65, 130)), ("lsq2", ((40, 8), (300, 70))), ("qp", ((300, 70), 130))]


@pytest.mark.parametrize("order", ["xu", "interleaved"])
@pytest.mark.parametrize("kind,shape", GENERIC, ids=[c[0] for c in GENERIC])
def test_against_the_generic_canonicalize(kind, shape, order):
    st, nx, nu = values(kind, shape, seed=21, positive=True)
    m, xv, uv = build(kind, st, nx, nu, order, None)
    ref, _, _ = build(kind, st, nx, nu, order, None, generic=True)
    try:
        gq, gl, gc = solved(m)
        rq, rl, rc = solved(ref)
        assert m.objective.mode == "canonical-groups"
        assert ref.objective.mode == "literal" and ref.objective.expr.builder == "canonicalize!"
        assert np.array_equal(gq["row"], rq["row"]) and np.array_equal(gq["col"], rq["col"])
        assert np.all(np.abs(gq["coeff"] - rq["coeff"]) <= 1e-12 * np.abs(rq["coeff"]))
        full = np.zeros(nx + nu)
        full[rl["var"] - 1] = rl["coeff"]                    # (the literal sum has no linear terms where a group has none)
        assert np.array_equal(gl["var"], np.arange(1, nx + nu + 1))
        assert np.all(np.abs(gl["coeff"] - full) <= 1e-12 * np.abs(full))
        assert abs(gc - rc) <= 1e-12 * abs(rc)
    finally:
        m.close()
        ref.close()
