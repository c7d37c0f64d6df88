"""Batched independent QPs sharded by instance across GPUs (BASELINE config 4).

In the reference a batch is many independent `Model`s (src/model.jl:1-22).  All instances share one structure, so a
re-evaluation produces one coefficient slab per instance (pmt_batch_lsq_coeffs_f64); rank g owns the contiguous instance
range shard_range(B, g, world) and ONE all-gather (RCCL over xGMI via torch.distributed) assembles every slab on every rank.
There is no other collective: the instances never interact.
"""
import ctypes as C
import json
import time

import numpy as np

from . import _lib
from ._lib import ArgumentError


def shard_range(total, rank, world):
    """Contiguous instance range [lo, hi) owned by `rank` (pmt_batch_shard): equal shards, or DimensionMismatch — the exchange lays the
    gathered buffer out as world * per_rank slabs, an uneven split would corrupt it silently."""
    per, first = C.c_int64(), C.c_int64()
    _lib.call("pmt_batch_shard", total, world, rank, C.byref(per), C.byref(first))
    return first.value, first.value + per.value


def slab_layout(n, m):
    """Offsets (in doubles) of the sections of one instance's slab and the slab length."""
    nq = n * (n + 1) // 2
    off = {"Q": 0, "q": nq, "const": nq + n, "C": nq + n + 1, "dconst": nq + n + 1 + m * n}
    return off, nq + n + 1 + m * n + m


def gather_slabs(dist, local, gathered):
    """all-gather of equally sized per-rank slab blocks into `gathered` ([world * B_local, L]); rank order = instance order."""
    if dist is None:
        gathered.copy_(local)
        return
    dist.all_gather_into_tensor(gathered.view(-1), local.contiguous().view(-1))


def chunk_schedule(per_rank, chunk):
    """The chunk schedule of pmt_batch_step_f64 / pmt_batch_allgather_f64 (the library's own host arithmetic, include/parametron_hip.h):
    [(lo, hi)] local instance ranges in exchange order; chunk <= 0 means one chunk."""
    L = _lib.load()
    out = []
    for c in range(int(L.pmt_batch_num_chunks(per_rank, chunk))):
        lo, hi = C.c_int64(), C.c_int64()
        _lib.call("pmt_batch_chunk_range", per_rank, chunk, c, C.byref(lo), C.byref(hi))
        out.append((lo.value, hi.value))
    return out


def gathered_offset(rank, per_rank, local_instance, stride):
    """position (in doubles) of a rank's local instance in the gathered buffer (global instance order)"""
    return int(_lib.load().pmt_batch_gathered_offset(rank, per_rank, local_instance, stride))


def exchange_chunks(dist, local, gathered, rank, world, chunk):
    """The library's exchange schedule driven through a torch.distributed backend that has no RCCL (the 2-rank gloo test on CPU): for
    every chunk, in order, one send / receive pair per peer (peers staggered as in comm.hip) and the local copy; `local` is
    [per_rank, stride], `gathered` [world * per_rank, stride]."""
    per_rank, stride = local.shape
    flat_l, flat_g = local.reshape(-1), gathered.reshape(-1)
    for lo, hi in chunk_schedule(per_rank, chunk):
        cnt = (hi - lo) * stride
        mine = gathered_offset(rank, per_rank, lo, stride)
        flat_g[mine:mine + cnt] = flat_l[lo * stride:lo * stride + cnt]
        if dist is None or world == 1:
            continue
        ops = []
        for k in range(1, world):
            to, frm = (rank + k) % world, (rank - k + world) % world
            off = gathered_offset(frm, per_rank, lo, stride)
            ops.append(dist.P2POp(dist.isend, flat_l[lo * stride:lo * stride + cnt].contiguous(), to))
            ops.append(dist.P2POp(dist.irecv, flat_g[off:off + cnt], frm))
        for req in dist.batch_isend_irecv(ops):
            req.wait()


class Communicator:
    """pmt_comm_*: the library's own RCCL communicator.  The launcher (torch.distributed here) only carries rank 0's unique id."""

    def __init__(self, torch, dist, rank, world, device_index, rccl_single=False):
        """rccl_single: a single rank still builds a real (one-rank) RCCL communicator and exchanges with itself — the N-rank code path on
        one GPU; False: a single rank loads no RCCL at all"""
        self.rank, self.world = rank, world
        self.handle = C.c_void_p()
        if world > 1:
            ident = (C.c_char * 128)()
            if rank == 0:
                _lib.call("pmt_comm_unique_id", C.cast(ident, C.c_void_p))
            t = torch.tensor(list(bytes(ident)), dtype=torch.uint8, device="cuda")
            dist.broadcast(t, src=0)
            ident = (C.c_char * 128).from_buffer_copy(bytes(t.cpu().tolist()))
            _lib.call("pmt_comm_init_rank", world, rank, C.cast(ident, C.c_void_p), device_index, C.byref(self.handle))
        elif rccl_single:
            ident = (C.c_char * 128)()
            _lib.call("pmt_comm_unique_id", C.cast(ident, C.c_void_p))
            _lib.call("pmt_comm_init_rank", 1, 0, C.cast(ident, C.c_void_p), device_index, C.byref(self.handle))
        else:
            _lib.call("pmt_comm_init_rank", 1, 0, None, device_index, C.byref(self.handle))

    def rccl_calls(self):
        return int(_lib.load().pmt_comm_rccl_calls(self.handle))

    def close(self):
        if self.handle:
            _lib.call("pmt_comm_destroy", self.handle)
            self.handle = C.c_void_p()


class _Batch:
    """What the batched workloads share: rank `rank` owns the instances shard_range(total, rank, world); every input is a flat device tensor
    of `per[name]` doubles per instance, generated by the counter-based stream — one stream per input and epoch, SEEDS[name] + 1000 * epoch,
    drawn at GLOBAL element offsets, so instance k holds the same data whatever the sharding; one row of `stride` doubles per instance in
    `local` (the slab of L doubles, and what a subclass appends behind it), all rows of all ranks in `gathered`.  A subclass names its
    inputs and their sizes, its layout, and its launch (compute)."""

    SEEDS = {}
    SCALES = {"d": 2.0}                          # the range of an input's stream where it is not 1.0
    ATTRS = {"C": "Cm", "B": "Bm"}               # an input is also an attribute of its name; C and B under these

    def __init__(self, torch, total, rank, world, device, per, layout):
        _lib.require_gpu()
        self.torch, self.total, self.rank, self.world = torch, total, rank, world
        self.lo, self.hi = shard_range(total, rank, world)
        self.B = self.hi - self.lo
        dev = device or torch.device("cuda", torch.cuda.current_device())
        self.per = per
        self.inputs = self._alloc(per, dev)
        self.offsets, self.L = layout
        self.stride = self.L + self._extra(dev)                  # doubles of one instance's row: the slab, and what a subclass appends
        self.local = torch.empty((self.B, self.stride), dtype=torch.float64, device=dev)
        self.gathered = torch.empty((total, self.stride), dtype=torch.float64, device=dev) if world > 1 else self.local
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.regenerate(0)

    @staticmethod
    def _p(t):
        return C.c_void_p(t.data_ptr())

    def _alloc(self, per, dev):
        """name -> tensor of B * per[name] doubles, each also set as the attribute of its name"""
        bufs = {k: self.torch.empty(self.B * cnt, dtype=self.torch.float64, device=dev) for k, cnt in per.items()}
        for k, t in bufs.items():
            setattr(self, self.ATTRS.get(k, k), t)
        return bufs

    def _extra(self, dev):
        """doubles a subclass appends to every instance's row behind the slab, after allocating its own inputs (_Dynamics)"""
        return 0

    def _fill(self, bufs, per, epoch):
        for name, buf in bufs.items():
            _lib.call("pmt_fill_uniform_offset_f64", self._p(buf), self.B * per[name], C.c_uint64(self.SEEDS[name] + 1000 * epoch),
                      C.c_uint64(self.lo * per[name]), self.SCALES.get(name, 1.0), self.stream)

    def regenerate(self, epoch):
        """device-side Parameter callbacks (↔ rand! in README.md:36-43), one stream per Parameter and epoch"""
        self._fill(self.inputs, self.per, epoch)

    def gather(self, dist):
        if self.world > 1:
            gather_slabs(dist, self.local, self.gathered)

    def step(self, dist):
        self.compute()
        self.gather(dist)


class BatchLSQ(_Batch):
    """Device-resident batch: A[B][r x n], b[B][r], C[B][m x n], d[B][m] generated by the counter-based stream so that
    instance k holds the same data whatever the sharding (seed streams are indexed by GLOBAL element index)."""

    SEEDS = {"A": 101, "b": 102, "C": 103, "d": 104}

    def __init__(self, torch, total, n, r, m, rank=0, world=1, device=None):
        self.n, self.r, self.m = n, r, m
        super().__init__(torch, total, rank, world, device, {"A": r * n, "b": r, "C": m * n, "d": m}, slab_layout(n, m))

    def compute(self):
        _lib.call("pmt_batch_lsq_coeffs_f64", self._p(self.A), self._p(self.b), self._p(self.Cm), self._p(self.d), self.B, self.n, self.r,
                  self.m, -1, -1, self._p(self.local), self.L, self.stream)

    def step_pipelined(self, comm, chunk):
        """pmt_batch_step_f64: compute chunk by chunk, chunk c on the wire (the library's RCCL communicator, its own stream) while
        chunk c + 1 is computed"""
        _lib.call("pmt_batch_step_f64", comm.handle, self._p(self.A), self._p(self.b), self._p(self.Cm), self._p(self.d), self.B, self.n, self.r,
                  self.m, -1, -1, self._p(self.local), self._p(self.gathered), self.L, int(chunk), self.stream)


class BatchTracking(_Batch):
    """Device-resident batch of tracking costs transpose(x - p_i) * Q_i * (x - p_i) over C_i*x == d_i (many small MPC instances, each with a
    weight matrix and a reference of its own): Q[B][n x n], p[B][n], C[B][m x n], d[B][m].  One launch of pmt_batch_form_coeffs_f64 writes
    the slabs, in the layout of BatchLSQ's — slab_layout, gather_slabs and pmt_batch_expand_f64 apply as they are.  There is no pipelined
    exchange for this objective (pmt_batch_step_f64 computes the least-squares slabs): step() is compute() and one all-gather."""

    SEEDS = {"Q": 201, "p": 202, "C": 203, "d": 204}

    def __init__(self, torch, total, n, m, rank=0, world=1, device=None):
        self.n, self.m = n, m
        super().__init__(torch, total, rank, world, device, {"Q": n * n, "p": n, "C": m * n, "d": m}, slab_layout(n, m))

    def compute(self):
        _lib.call("pmt_batch_form_coeffs_f64", self._p(self.Q), self._p(self.p), self._p(self.Cm), self._p(self.d), self.B, self.n, self.m,
                  -1, -1, self._p(self.local), self.L, self.stream)


def horizon_sizes(T, nx, nu, term=0):
    """What every horizon layout counts: (nqx, nqu, n, ns) — the words of the upper triangle of an nx x nx and of an nu x nu matrix, the
    n = T*(nx + nu) + term*nx variables of z, the ns = T*(1 + (nu > 0)) + term stages in z order."""
    return nx * (nx + 1) // 2, nu * (nu + 1) // 2, T * (nx + nu) + term * nx, T * (2 if nu else 1) + term


def horizon_slab_layout(T, nx, nu, m):
    """Offsets (in doubles) of the sections of one horizon instance's slab [SQ | SR | q | const | C | d-consts] over n = T*(nx + nu)
    variables, and the slab length (pmt_batch_horizon_slab_doubles)."""
    nqx, nqu, n, _ = horizon_sizes(T, nx, nu)
    q = nqx + nqu
    off = {"SQ": 0, "SR": nqx, "q": q, "const": q + n, "C": q + n + 1, "dconst": q + n + 1 + m * n}
    return off, q + n + 1 + m * n + m


class _HorizonBatch(_Batch):
    """The horizon workloads: T stages of nx states and nu inputs, `term` terminal stages x_T behind them, n variables in z.  A subclass
    names the entry point that expands a slab (EXPAND) and the dimensions it takes (_expand_dims)."""

    term = 0

    def __init__(self, torch, total, T, nx, nu, m, rank, world, device, per, layout):
        self.T, self.nx, self.nu, self.m = T, nx, nu, m
        super().__init__(torch, total, rank, world, device, per, layout)

    def expand(self, i, xvar, varmap):
        """the MOI buffers of local instance i from its slab (EXPAND): xvar the n model variables of z, varmap the model-to-optimizer index
        map, both int64 device tensors -> (quadratic terms as 3 words each, linear terms as 2 words each, the constant, vector-affine terms
        as 3 words each, their m constants), device tensors"""
        torch, n, m = self.torch, self.n, self.m
        nqx = self.nx * (self.nx + 1) // 2
        nq = self.T * (nqx + self.nu * (self.nu + 1) // 2) + self.term * nqx
        dev = self.local.device
        quad = torch.empty(3 * nq, dtype=torch.int64, device=dev)
        lin = torch.empty(2 * n, dtype=torch.int64, device=dev)
        const = torch.empty(1, dtype=torch.float64, device=dev)
        vat = torch.empty(max(3 * m * n, 1), dtype=torch.int64, device=dev)
        vconsts = torch.empty(max(m, 1), dtype=torch.float64, device=dev)
        _lib.call(self.EXPAND, C.c_void_p(self.local.data_ptr() + 8 * i * self.stride), *self._expand_dims(), self._p(xvar), self._p(varmap),
                  self._p(quad), self._p(lin), self._p(const), self._p(vat), self._p(vconsts), self.stream)
        return quad, lin, const, vat[:3 * m * n], vconsts[:m]


class BatchHorizon(_HorizonBatch):
    """Device-resident batch of MPC horizons sum_t transpose(x_t - r_{i,t}) * Q_i * (x_t - r_{i,t}) + transpose(u_t) * R_i * u_t over
    C_i*z == d_i, z = [x_0; u_0; x_1; ..] (a fleet of controllers, or of sampled scenarios: every instance with weights and stage references
    of its own): Q[B][nx x nx], R[B][nu x nu], r[B][T x nx], v[B][T x nu], C[B][m x n], d[B][m].  One launch of
    pmt_batch_horizon_coeffs_f64 writes the slabs (horizon_slab_layout); gather_slabs takes them as they are; expand() rebuilds one
    instance's MOI buffers.  There is no pipelined exchange for this objective: step() is compute() and one all-gather."""

    SEEDS = {"Q": 301, "R": 302, "r": 303, "v": 304, "C": 305, "d": 306}
    EXPAND = "pmt_batch_horizon_expand_f64"

    def __init__(self, torch, total, T, nx, nu, m, rank=0, world=1, device=None):
        self.n = T * (nx + nu)
        layout = horizon_slab_layout(T, nx, nu, m)
        assert layout[1] == _lib.load().pmt_batch_horizon_slab_doubles(T, nx, nu, m)
        super().__init__(torch, total, T, nx, nu, m, rank, world, device,
                         {"Q": nx * nx, "R": nu * nu, "r": T * nx, "v": T * nu, "C": m * self.n, "d": m}, layout)

    def compute(self):
        """x_t - r_t, u_t as it is, C*z - d"""
        _lib.call("pmt_batch_horizon_coeffs_f64", self._p(self.Q), self._p(self.R), self._p(self.r), self._p(self.v), self._p(self.Cm),
                  self._p(self.d), self.B, self.T, self.nx, self.nu, self.m, -1, 0, -1, self._p(self.local), self.stride, self.stream)

    def _expand_dims(self):
        return self.T, self.nx, self.nu, self.m


def horizon_dynamics_layout(T, nx, nu):
    """Offsets (in doubles) of the sections of one horizon instance's dynamics section [AB | h-consts] — AB the nx rows of [A_i | B_i],
    row-major with row length nx + nu, then the T*nx record constants — and its length Ld (pmt_batch_horizon_dynamics_doubles)."""
    nab = nx * (nx + nu)
    return {"AB": 0, "hconst": nab}, nab + T * nx


class _DynamicsRows:
    """A horizon workload with dynamics rows of the instances' own in Td = T + term records: A, B and h[B][Td x nx] beside the sibling's
    inputs (not among `inputs`: those are the sibling's), with seeds of their own and drawn at global element offsets like every input.
    One row per instance, [slab (L) | dynamics section]: compute() is the sibling's launch at the row's stride and one launch of DYN_COEFFS
    on the same stream; gather_slabs moves the rows as they are; expand() adds the Td records' terms and constants (DYN_EXPAND: it reads no
    variable past x_{Td-1}) to the sibling's five buffers.  A subclass names the two entry points, the section's layout function with the
    attribute that holds its length, and how many [A | B] pairs an instance has."""

    DYN_COEFFS = DYN_EXPAND = DYN_LAYOUT = None

    def _extra(self, dev):
        nx, nu = self.nx, self.nu
        self.Td = self.T + self.term
        pairs = self._pairs()
        self.dyn_per = {"A": pairs * nx * nx, "B": pairs * nx * nu, "h": self.Td * nx}
        self.dyn_inputs = self._alloc(self.dyn_per, dev)
        layout, length = self.DYN_LAYOUT
        self.dyn_offsets, Ld = layout(self.Td, nx, nu)
        assert Ld == getattr(_lib.load(), self.DYN_COEFFS.replace("_f64", "_doubles"))(self.Td, nx, nu)
        setattr(self, length, Ld)
        return Ld

    def regenerate(self, epoch):
        super().regenerate(epoch)
        self._fill(self.dyn_inputs, self.dyn_per, epoch)

    def compute(self):
        """the sibling's slab, and behind it x_t - A*x_{t-1} - B*u_{t-1} - h_t for t = 1 .. Td-1 (A, B the stage's own where they vary)"""
        super().compute()
        _lib.call(self.DYN_COEFFS, self._p(self.A), self._p(self.Bm), self._p(self.h), self.B, self.Td, self.nx, self.nu, -1, -1, -1,
                  C.c_void_p(self.local.data_ptr() + 8 * self.L), self.stride, self.stream)

    def expand(self, i, xvar, varmap):
        """the sibling's five buffers of local instance i, then the dynamics records' vector-affine terms (3 words each) and constants"""
        torch, Td, nx, w = self.torch, self.Td, self.nx, self.nx + self.nu
        dev = self.local.device
        terms = torch.empty(3 * (nx + (Td - 1) * nx * (1 + w)), dtype=torch.int64, device=dev)
        consts = torch.empty(Td * nx, dtype=torch.float64, device=dev)
        five = super().expand(i, xvar, varmap)
        _lib.call(self.DYN_EXPAND, C.c_void_p(self.local.data_ptr() + 8 * (i * self.stride + self.L)), Td, nx, self.nu, 1, self._p(xvar),
                  self._p(varmap), self._p(terms), self._p(consts), self.stream)
        return five + (terms, consts)


class _Dynamics(_DynamicsRows):
    """_DynamicsRows with one pair per instance, x_0 == h_{i,0}, x_t == A_i*x_{t-1} + B_i*u_{t-1} + h_{i,t}: A[B][nx x nx], B[B][nx x nu]; the
    section [AB | h-consts] of Ld doubles."""

    DYN_COEFFS, DYN_EXPAND = "pmt_batch_horizon_dynamics_f64", "pmt_batch_horizon_dynamics_expand_f64"
    DYN_LAYOUT = (horizon_dynamics_layout, "Ld")

    def _pairs(self):
        return 1


class BatchMPC(_Dynamics, BatchHorizon):
    """BatchHorizon with the instances' own dynamics (_Dynamics, Td = T records).  m counts further dense rows C_i*z == d_i (default: none)."""

    SEEDS = dict(BatchHorizon.SEEDS, A=307, B=308, h=309)

    def __init__(self, torch, total, T, nx, nu, m=0, rank=0, world=1, device=None):
        super().__init__(torch, total, T, nx, nu, m, rank, world, device)


def horizon_dynamics_tv_layout(T, nx, nu):
    """Offsets (in doubles) of the sections of one horizon instance's time-varying dynamics section [AB_1 | .. | AB_{T-1} | h-consts] —
    "AB" the list of the T - 1 blocks' offsets (AB_t at index t - 1: the nx rows of [A_{i,t} | B_{i,t}], row-major with row length nx + nu),
    then the T*nx record constants — and its length Ltv (pmt_batch_horizon_dynamics_tv_doubles)."""
    nab = nx * (nx + nu)
    Ltv = (T - 1) * nab + T * nx
    assert Ltv == _lib.load().pmt_batch_horizon_dynamics_tv_doubles(T, nx, nu)
    return {"AB": [s * nab for s in range(T - 1)], "hconst": (T - 1) * nab}, Ltv


class _TimeVaryingDynamics(_DynamicsRows):
    """_DynamicsRows with a pair per stage, x_0 == h_{i,0}, x_t == A_{i,t}*x_{t-1} + B_{i,t}*u_{t-1} + h_{i,t} (the fleet that re-linearises
    every stage at every solve): A[B][Td-1][nx x nx], B[B][Td-1][nx x nu]; the section [AB_1 | .. | AB_{Td-1} | h-consts] of Ltv doubles."""

    DYN_COEFFS, DYN_EXPAND = "pmt_batch_horizon_dynamics_tv_f64", "pmt_batch_horizon_dynamics_tv_expand_f64"
    DYN_LAYOUT = (horizon_dynamics_tv_layout, "Ltv")

    def _pairs(self):
        return self.Td - 1


class BatchLTVMPC(_TimeVaryingDynamics, BatchHorizon):
    """BatchHorizon with dynamics of its own per instance and stage (_TimeVaryingDynamics, Td = T records).  m counts further dense rows
    C_i*z == d_i (default: none)."""

    SEEDS = dict(BatchHorizon.SEEDS, A=310, B=311, h=312)

    def __init__(self, torch, total, T, nx, nu, m=0, rank=0, world=1, device=None):
        super().__init__(torch, total, T, nx, nu, m, rank, world, device)


def horizon_terms_slab_layout(T, nx, nu, m, terminal):
    """Offsets (in doubles) of the sections of one weighted horizon instance's slab [SQ | SR | SP | W | q | const | C | d-consts] over
    n = T*(nx + nu) + term*nx variables — SP only with a terminal stage, W the ns = T*(1 + (nu > 0)) + term stage weights in z order — and
    the slab length (pmt_batch_horizon_terms_slab_doubles)."""
    term = 1 if terminal else 0
    nqx, nqu, n, ns = horizon_sizes(T, nx, nu, term)
    w0 = nqx + nqu + term * nqx
    q = w0 + ns
    off = {"SQ": 0, "SR": nqx, "SP": nqx + nqu, "W": w0, "q": q, "const": q + n, "C": q + n + 1, "dconst": q + n + 1 + m * n}
    L = q + n + 1 + m * n + m
    assert L == _lib.load().pmt_batch_horizon_terms_slab_doubles(T, nx, nu, term, m)
    return off, L


class BatchWeightedHorizon(_HorizonBatch):
    """Device-resident batch of MPC horizons with a terminal cost, stage weights and linear stage terms,
        sum_t wx_{i,t} * transpose(x_t - r_{i,t}) * Q_i * (x_t - r_{i,t}) + dot(gx_{i,t}, x_t) + wu_{i,t} * transpose(u_t) * R_i * u_t + dot(gu_{i,t}, u_t)
        + wN_i * transpose(x_T - rN_i) * P_i * (x_T - rN_i) + dot(gN_i, x_T)
    over C_i*z == d_i, z = [x_0; u_0; ..; u_{T-1}; x_T]: the sibling of BatchHorizon for fleets whose objectives carry a discount or a scenario
    probability per stage, an economic term, a terminal matrix.  `terminal` adds P, rN (and x_T to z), `weights` the arrays wx, wu, wN,
    `linear` the arrays gx, gu, gN; `signs` = (sign_r, sign_v, sign_rN, sign_d), a reference with sign 0 is not allocated.  All inputs have
    seeds of their own.  One launch of pmt_batch_horizon_terms_coeffs_f64 writes the slabs (horizon_terms_slab_layout); gather_slabs takes
    them as they are; expand() rebuilds one instance's MOI buffers.  There is no pipelined exchange for this objective: step() is compute()
    and one all-gather."""

    SEEDS = {"Q": 401, "R": 402, "P": 403, "r": 404, "v": 405, "rN": 406, "wx": 407, "wu": 408, "wN": 409, "gx": 410, "gu": 411, "gN": 412,
             "C": 413, "d": 414}
    EXPAND = "pmt_batch_horizon_terms_expand_f64"

    def __init__(self, torch, total, T, nx, nu, m, terminal=True, weights=True, linear=True, signs=(-1, 0, -1, -1), rank=0, world=1, device=None):
        self.term = 1 if terminal else 0
        self.n = T * (nx + nu) + self.term * nx
        self.signs = dict(zip(("r", "v", "rN", "d"), signs))
        per = {"Q": nx * nx, "R": nu * nu, "C": m * self.n, "d": m}
        if self.signs["r"]:
            per["r"] = T * nx
        if self.signs["v"] and nu:
            per["v"] = T * nu
        if terminal:
            per["P"] = nx * nx
            if self.signs["rN"]:
                per["rN"] = nx
        if weights:
            per.update({"wx": T, "wu": T if nu else 0}, **({"wN": 1} if terminal else {}))
        if linear:
            per.update({"gx": T * nx, "gu": T * nu}, **({"gN": nx} if terminal else {}))
        super().__init__(torch, total, T, nx, nu, m, rank, world, device, per, horizon_terms_slab_layout(T, nx, nu, m, terminal))

    def descriptor(self):
        """the pmt_batch_horizon_terms of this shard's inputs"""
        ptrs = {k: (buf.data_ptr() if self.per[k] else None) for k, buf in self.inputs.items()}
        return _lib.batch_horizon_terms(sign_r=self.signs["r"], sign_v=self.signs["v"], sign_rN=self.signs["rN"], sign_d=self.signs["d"], **ptrs)

    def compute(self):
        desc = self.descriptor()
        _lib.call("pmt_batch_horizon_terms_coeffs_f64", C.byref(desc), self.B, self.T, self.nx, self.nu, self.m, self._p(self.local), self.stride,
                  self.stream)

    def _expand_dims(self):
        return self.T, self.nx, self.nu, self.term, self.m


class BatchWeightedMPC(_Dynamics, BatchWeightedHorizon):
    """BatchWeightedHorizon with the instances' own dynamics (_Dynamics), as BatchMPC is BatchHorizon with them.  With a terminal stage the
    dynamics have Td = T + 1 records, up to x_T == A_i*x_{T-1} + B_i*u_{T-1} + h_{i,T} (so T <= 511 then); without one Td = T.  m counts
    further dense rows C_i*z == d_i (default: none)."""

    SEEDS = dict(BatchWeightedHorizon.SEEDS, A=415, B=416, h=417)

    def __init__(self, torch, total, T, nx, nu, m=0, terminal=True, weights=True, linear=True, signs=(-1, 0, -1, -1), rank=0, world=1, device=None):
        super().__init__(torch, total, T, nx, nu, m, terminal, weights, linear, signs, rank, world, device)


class BatchWeightedLTVMPC(_TimeVaryingDynamics, BatchWeightedHorizon):
    """BatchWeightedHorizon with dynamics of its own per instance and stage (_TimeVaryingDynamics), as BatchLTVMPC is BatchHorizon with them.
    With a terminal stage the dynamics have Td = T + 1 records, up to x_T == A_{i,T}*x_{T-1} + B_{i,T}*u_{T-1} + h_{i,T} (so T <= 511 then);
    without one Td = T.  m counts further dense rows C_i*z == d_i (default: none)."""

    SEEDS = dict(BatchWeightedHorizon.SEEDS, A=418, B=419, h=420)

    def __init__(self, torch, total, T, nx, nu, m=0, terminal=True, weights=True, linear=True, signs=(-1, 0, -1, -1), rank=0, world=1, device=None):
        super().__init__(torch, total, T, nx, nu, m, terminal, weights, linear, signs, rank, world, device)


def horizon_tv_slab_layout(T, nx, nu, m, terminal):
    """Offsets (in doubles) of the sections of one instance's slab [S | q | sconst | const | C | d-consts] of a horizon with a weight matrix
    per stage, over n = T*(nx + nu) + term*nx variables — "S" the list of the ns = T*(1 + (nu > 0)) + term blocks' offsets in z order
    (x_0, u_0, x_1, .., x_T; block s holds nd(nd+1)/2 words, nd = nx or nu), sconst the ns stage constants — and the slab length
    (pmt_batch_horizon_tv_slab_doubles)."""
    term = 1 if terminal else 0
    nqx, nqu, n, ns = horizon_sizes(T, nx, nu, term)
    blocks = []
    for t in range(T + term):
        blocks.append(t * (nqx + nqu))
        if nu and t < T:
            blocks.append(t * (nqx + nqu) + nqx)
    q = T * (nqx + nqu) + term * nqx
    off = {"S": blocks, "q": q, "sconst": q + n, "const": q + n + ns, "C": q + n + ns + 1, "dconst": q + n + ns + 1 + m * n}
    L = q + n + ns + 1 + m * n + m
    assert L == _lib.load().pmt_batch_horizon_tv_slab_doubles(T, nx, nu, term, m)
    return off, L


class BatchTVHorizon(_HorizonBatch):
    """Device-resident batch of MPC horizons whose stage weights change with the stage,
        sum_t transpose(x_t - r_{i,t}) * Q_{i,t} * (x_t - r_{i,t}) + transpose(u_t) * R_{i,t} * u_t  [+ transpose(x_T - r_{i,T}) * Q_{i,T} * (x_T - r_{i,T})]
    over C_i*z == d_i, z = [x_0; u_0; ..; u_{T-1}; (x_T)] — the fleet that re-linearises its cost at every stage and solve (a Gauss-Newton or
    exact Hessian block per stage): Q[B][T+term][nx x nx], R[B][T][nu x nu], r[B][T+term][nx], v[B][T][nu], C[B][m x n], d[B][m].
    `terminal` adds the stage x_T with a matrix and a reference of its own.  pmt_batch_horizon_tv_coeffs_f64 writes the slabs
    (horizon_tv_slab_layout); gather_slabs takes them as they are; expand() rebuilds one instance's MOI buffers.  There is no pipelined
    exchange for this objective: step() is compute() and one all-gather."""

    SEEDS = {"Q": 501, "R": 502, "r": 503, "v": 504, "C": 505, "d": 506}
    EXPAND = "pmt_batch_horizon_tv_expand_f64"

    def __init__(self, torch, total, T, nx, nu, m, terminal=False, rank=0, world=1, device=None):
        self.term = 1 if terminal else 0
        self.n = T * (nx + nu) + self.term * nx
        Tx = T + self.term
        super().__init__(torch, total, T, nx, nu, m, rank, world, device,
                         {"Q": Tx * nx * nx, "R": T * nu * nu, "r": Tx * nx, "v": T * nu, "C": m * self.n, "d": m},
                         horizon_tv_slab_layout(T, nx, nu, m, terminal))

    def compute(self):
        """x_t - r_t, u_t as it is, C*z - d"""
        _lib.call("pmt_batch_horizon_tv_coeffs_f64", self._p(self.Q), self._p(self.R), self._p(self.r), self._p(self.v), self._p(self.Cm),
                  self._p(self.d), self.B, self.T, self.nx, self.nu, self.term, self.m, -1, 0, -1, self._p(self.local), self.stride, self.stream)

    def _expand_dims(self):
        return self.T, self.nx, self.nu, self.term, self.m


class BatchTVMPC(_TimeVaryingDynamics, BatchTVHorizon):
    """BatchTVHorizon with dynamics of its own per instance and stage (_TimeVaryingDynamics): time-varying weights and time-varying dynamics
    in one row [slab | Ltv].  With a terminal stage the dynamics have Td = T + 1 records, up to x_T == A_{i,T}*x_{T-1} + B_{i,T}*u_{T-1} +
    h_{i,T} (so T <= 511 then); without one Td = T.  m counts further dense rows C_i*z == d_i (default: none)."""

    SEEDS = dict(BatchTVHorizon.SEEDS, A=507, B=508, h=509)

    def __init__(self, torch, total, T, nx, nu, m=0, terminal=False, rank=0, world=1, device=None):
        super().__init__(torch, total, T, nx, nu, m, terminal, rank, world, device)


TOTAL, N, R, M = 8192, 128, 128, 16      # BASELINE config 4 (m is not stated there: 16)


def sharded_report(world, ranks_seen, steps, warmup, t_pipe, t_mono, t_compute, nchunks, total=TOTAL, n=N, r=R, m=M):
    """The JSON object of the sharded C4 step (pure arithmetic on the three measured times: testable without a GPU).
    value = the whole job's instances per second with the exchange overlapped; beside it compute-only and computation + one monolithic
    all-gather, the bytes every rank puts on the wire and what a per-link-bound exchange of them would cost."""
    off, L = slab_layout(n, m)
    per_inst_bytes = 8.0 * (r * n + r + m * n + m) + 8.0 * L
    per_gpu = per_inst_bytes * (total // world)
    exch = 8.0 * L * (total // world)
    return {
        "metric": "QP re-evaluations/sec (Q,q,C,d rebuild), batched n=128", "value": total * steps / t_pipe,
        "unit": "re-evaluations/s", "n_gpus": world, "ranks_seen": ranks_seen, "steps": steps, "warmup": warmup,
        "ms_per_step": t_pipe / steps * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic",
        "config": {"workload": "C4 batch of 8192 independent QPs n=r=128 m=16, sharded by instance; value = computation + chunked "
                               "exchange of the coefficient slabs overlapped (pmt_batch_step_f64: RCCL send/recv per peer behind the C ABI)",
                   "instances": total, "instances_per_gpu": total // world, "slab_doubles": L, "exchange_chunks_per_rank": nchunks,
                   "parallelism": "instance sharding + direct (per-peer) exchange over xGMI" if world > 1 else "single GPU (single-rank communicator, same code path)"},
        "compute_only": {"value": total * steps / t_compute, "ms_per_step": t_compute / steps * 1e3},
        "compute_then_allgather": {"value": total * steps / t_mono, "ms_per_step": t_mono / steps * 1e3,
                                   "what": "one torch.distributed all_gather_into_tensor behind the computation (round 1's path)"},
        "compute_overlapped_exchange": {"value": total * steps / t_pipe, "ms_per_step": t_pipe / steps * 1e3},
        "exchange_bytes_per_rank": exch, "step_algorithmic_bytes_per_gpu": per_gpu,
        "expected_exchange_ms": {"direct_per_link": exch / 153e9 * 1e3 if world > 1 else 0.0,
                                 "ring": (world - 1) * exch / 153e9 * 1e3 if world > 1 else 0.0,
                                 "note": "xGMI ~153 GB/s per link, 7 links per GPU (MI355X_MICROARCH.md): direct = every peer over its own link"},
        "roofline": {"kernel": "batch_small_kernel", "bound": "hbm", "achieved": per_gpu / (t_compute / steps) / 1e9, "peak": 8000.0, "unit": "GB/s",
                     "frac": per_gpu / (t_compute / steps) / 1e9 / 8000.0, "traffic": None,
                     "note": "compute-only step (one batch_small_kernel launch per step); both bounds of the step are ~0.3 ms at 1 GPU"},
        "cpu_baseline": None,
    }


def measure(torch, dist, rank, world, steps, warmup):
    """The sharded C4 step on `world` ranks (every rank calls this; world == 1: the same code path with the single-rank communicator).
    Times K steps three ways — exchange overlapped (pmt_batch_step_f64), monolithic all-gather behind the computation, computation only —
    each bracketed by barrier + synchronize, MAX over ranks.  Returns the report on rank 0, None elsewhere."""
    wl = BatchLSQ(torch, TOTAL, N, R, M, rank, world)
    comm = Communicator(torch, dist, rank, world, torch.cuda.current_device())
    # one rank: nothing to exchange, one launch.  Several ranks: the first exchange starts after 1/8 of the computation, but a chunk never
    # has fewer instances than the GPU has CUs (batch_small_kernel is one persistent workgroup per CU)
    chunk = wl.B if world == 1 else max(256, wl.B // 8)

    def timed(fn):
        torch.cuda.synchronize()
        if dist:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0          # this rank's K steps are complete; the MAX over ranks below is the job's time
        if dist:
            dist.barrier()
        torch.cuda.synchronize()
        if dist:
            t = torch.tensor([el], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        return el

    for _ in range(max(warmup, 60)):                       # >= 30 ms of work: the clock settles before anything is timed
        wl.compute()
    for _ in range(3):
        wl.step(dist)
        wl.step_pipelined(comm, chunk)
    t_pipe = timed(lambda: wl.step_pipelined(comm, chunk))
    t_mono = timed(lambda: wl.step(dist))
    t_compute = timed(wl.compute)
    ranks_seen = world
    if dist:
        one = torch.ones(1, dtype=torch.int64, device="cuda")
        dist.all_reduce(one)
        ranks_seen = int(one.item())
    nchunks = len(chunk_schedule(wl.B, chunk))
    rccl_calls = comm.rccl_calls()
    comm.close()
    rep = sharded_report(world, ranks_seen, steps, warmup, t_pipe, t_mono, t_compute, nchunks) if rank == 0 else None
    if world == 1:
        # One GPU: the value above loads no RCCL (a single rank has nothing to exchange).  The library's RCCL binding is exercised all the
        # same: a real ONE-RANK communicator (ncclGetUniqueId / ncclCommInitRank) whose chunks travel to itself through grouped ncclSend /
        # ncclRecv on the communication stream — the N-rank code path on this GPU, checked against the plain result and timed beside it.
        try:
            want = wl.local.clone()
            c1 = Communicator(torch, None, 0, 1, torch.cuda.current_device(), rccl_single=True)
            wl.gathered = torch.full_like(wl.local, float("nan"))
            ch = max(256, wl.B // 8)
            for _ in range(3):
                wl.step_pipelined(c1, ch)
            torch.cuda.synchronize()
            ok = bool(torch.equal(wl.gathered, want) and torch.equal(wl.local, want))
            t_self = timed(lambda: wl.step_pipelined(c1, ch))
            rccl_calls = c1.rccl_calls()
            c1.close()
            rep["rccl_self_exchange"] = {"ms_per_step": t_self / steps * 1e3, "chunks": len(chunk_schedule(wl.B, ch)), "gathered_equals_local": ok,
                                         "what": "one-rank RCCL communicator: every chunk sent to / received from this rank through RCCL while the next is computed"}
        except Exception as e:
            rep["rccl_self_exchange"] = {"error": "%s: %s" % (type(e).__name__, e)}
    if rep is not None:
        rep["rccl_calls_made"] = rccl_calls > 0
        rep["rccl_calls"] = rccl_calls
    return rep


def bench(args, torch, dist, lib_mod, rank, world, emit=None):
    """bench.py --workload batch: 8192 x (n = r = 128, m = 16) instances, strong scaling over ranks.  Reports the re-evaluation rate
    compute-only, with one monolithic all-gather behind the computation (torch.distributed), and with the library's chunked exchange
    overlapped with the computation (pmt_batch_step_f64) — BASELINE.md §3 asks for the gather included and excluded."""
    out = measure(torch, dist, rank, world, args.steps, args.warmup)
    if rank == 0:
        (emit or (lambda o: print(json.dumps(o), flush=True)))(out)        # (bench.py passes the writer that owns the real stdout)
    if dist:
        dist.barrier()
        dist.destroy_process_group()
