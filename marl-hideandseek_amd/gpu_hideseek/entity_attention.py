"""The reference's other network: EntitySelfAttentionNet(num_embed_channels=128, num_out_channels=256, num_heads=4), which
scripts/jax_policy.py can build its ActorNet and CriticNet from in place of SimpleNet.  Every entity of a packed row is a
token, the 17 tokens attend to each other, and the result is pooled: what max-pooling each table on its own cannot
express, "the box between me and that seeker".

The projections are GEMMs and stay with torch (the matrix cores).  What sits between the QKV GEMM and the output GEMM,
per row 4 heads of 17 queries over at most 17 keys, is one kernel each way (hs_entity_attend,
hs_entity_attend_backward, csrc/hs_k_attend.h); include/hideseek.h states its arithmetic, IEEE f32 in a fixed order.
madrona_learn is not part of the reference's tree, so the network below is the project's own, modelled on the
reference's call and its three sizes, and pinned by nothing outside this repository.

    enc = entity_attention.AttentionEncoder(embed=128, out=256).cuda()
    feats = enc(sim, rows, torch.bfloat16, masked=True)                # [n, 256], part of the autograd graph
    out = sim.attend_entities(qkv, key_mask)["out"]                    # the core alone: qkv [n, 17, 3, 4, D] -> [n, 17, E]

eager() is the same function in plain torch, for readers, tools/attend_bench.py and the tests;
AttentionEncoder(..., fused=False) runs every piece's eager() on the same parameters.

The kernel reads and writes pieces of 4 adjacent elements, so qkv, out, grad_out and grad_qkv must be 16-byte aligned.
"""
import ctypes as C
import functools
import math

from . import mlp
from ._request import _DTYPES, _OUTPUT, _dtype_arg, _module_base, _name, _outputs, _run, _shard_calls, _tensor, _wanted
from .policy_inputs import TABLES

TOKENS = sum(math.prod(shape[:-1]) for _, _, shape in TABLES.values())      # HS_ATTEND_TOKENS: self, 5 agents, 9 boxes, 2 ramps
HEADS = 4                 # HS_ATTEND_HEADS
EMBED_DIMS = (64, 128)    # E = HEADS * D
ALIGN = 16                # bytes: qkv, out, grad_out and grad_qkv
ROWS_PER_ROUND = 4        # HS_ATTEND_ROWS_PER_ROUND: one row per wave, four waves
MAX_GRID = 2048           # HS_ATTEND_MAX_GRID: workgroups of a call at the most
MAX_ROWS = 1 << 24        # HS_ATTEND_MAX_ROWS
INDEX_LIMIT = 1 << 31     # hs_dense_norm_act indexes its [n, C] in int32: AttentionEncoder keeps rows * 17 * E of one call below it


class HsEntityAttendRequest(C.Structure):
    """hs_entity_attend_request (include/hideseek.h)."""
    _fields_ = [("qkv", C.c_void_p), ("key_mask", C.c_void_p), ("n", C.c_int32), ("embed_dim", C.c_int32), ("qkv_dtype", C.c_int32),
                ("out_dtype", C.c_int32), ("out", C.c_void_p)]


class HsEntityAttendBackwardRequest(C.Structure):
    """hs_entity_attend_backward_request (include/hideseek.h)."""
    _fields_ = [("qkv", C.c_void_p), ("key_mask", C.c_void_p), ("grad_out", C.c_void_p), ("n", C.c_int32), ("embed_dim", C.c_int32),
                ("qkv_dtype", C.c_int32), ("grad_dtype", C.c_int32), ("grad_qkv", C.c_void_p)]


def table_tokens():
    """[(table, first token, count, features per entity)] in token order: the entities of policy_inputs.TABLES."""
    out, first = [], 0
    for name, (_, _, shape) in TABLES.items():
        count = math.prod(shape[:-1])
        out.append((name, first, count, shape[-1]))
        first += count
    return out


def eager(qkv, key_mask=None):
    """The plain-torch function in qkv's dtype (float32 or float64; a narrower one is computed in float32):
    out [n, 17, E] of qkv [n, 17, 3, 4, D] and key_mask [n, 17] (nonzero = valid) or None.  Token 0 is always valid; a
    masked key's k and v are not looked at.  Differentiable in qkv."""
    import torch
    dt = qkv.dtype if qkv.dtype in (torch.float32, torch.float64) else torch.float32
    n, S, _, H, D = qkv.shape
    q, k, v = qkv.to(dt).unbind(2)                                            # [n, S, H, D]
    if key_mask is not None:
        valid = key_mask != 0
        valid = torch.cat([torch.ones_like(valid[:, :1]), valid[:, 1:]], 1)
        k = torch.where(valid[:, :, None, None], k, torch.zeros_like(k))
        v = torch.where(valid[:, :, None, None], v, torch.zeros_like(v))
    s = torch.einsum("nihd,njhd->nhij", q, k) * (1.0 / math.sqrt(D))
    if key_mask is not None:
        s = s.masked_fill(~valid[:, None, None, :], float("-inf"))
    p = torch.softmax(s, -1)
    return torch.einsum("nhij,njhd->nihd", p, v).reshape(n, S, H * D)


# ---- the fused calls ----
_QKV_SHAPES = [("n >= 1", TOKENS, 3, HEADS, E // HEADS) for E in EMBED_DIMS]


def _common(gpu_id, qkv, key_mask):
    import torch
    dev = torch.device("cuda", gpu_id)
    _tensor("qkv", qkv, _QKV_SHAPES, _DTYPES, dev, align=ALIGN)
    n, E = int(qkv.shape[0]), HEADS * int(qkv.shape[4])
    if n >= MAX_ROWS:
        raise ValueError(f"qkv must have fewer than {MAX_ROWS} rows, got {n}")
    inputs = [("qkv", qkv)]
    if key_mask is not None:
        _tensor("key_mask", key_mask, (n, TOKENS), ("uint8",), dev, "None or a torch tensor")
        inputs.append(("key_mask", key_mask))
    return dev, n, E, inputs


def _aligned_out(shape, dtypes, dev):
    return lambda k, t: _tensor(k, t, shape, dtypes, dev, _OUTPUT, align=ALIGN)


def request(gpu_id, qkv, key_mask=None, out=True, out_dtype=None):
    """Validate a forward call over the n = qkv.shape[0] rows on GPU `gpu_id`, allocate out when given as True (in
    `out_dtype`, by default qkv's), and return ({"out": tensor}, HsEntityAttendRequest).  Raises ValueError before the
    library is involved."""
    dev, n, E, inputs = _common(gpu_id, qkv, key_mask)
    outputs = _wanted((("out", out),), "out not requested")
    _dtype_arg("out_dtype", out_dtype)
    shape = (n, TOKENS, E)
    res, ptr = _outputs(outputs, {"out": (shape, qkv.dtype if out_dtype is None else out_dtype, _aligned_out(shape, _DTYPES, dev))}, inputs, dev)
    req = HsEntityAttendRequest(qkv.data_ptr(), None if key_mask is None else key_mask.data_ptr(), n, E, _DTYPES[_name(qkv.dtype)],
                                _DTYPES[_name(res["out"].dtype)], ptr("out"))
    return res, req


def request_backward(gpu_id, qkv, key_mask, grad_out, grad_qkv=True):
    """Validate a backward call, allocate grad_qkv when given as True (in grad_out's dtype, as a tensor given must be),
    and return ({"grad_qkv": tensor}, HsEntityAttendBackwardRequest).  Raises ValueError before the library is involved."""
    dev, n, E, inputs = _common(gpu_id, qkv, key_mask)
    _tensor("grad_out", grad_out, (n, TOKENS, E), _DTYPES, dev, align=ALIGN)
    inputs.append(("grad_out", grad_out))
    outputs = _wanted((("grad_qkv", grad_qkv),), "grad_qkv not requested")
    shape = tuple(qkv.shape)
    res, ptr = _outputs(outputs, {"grad_qkv": (shape, grad_out.dtype, _aligned_out(shape, (_name(grad_out.dtype),), dev))}, inputs, dev)
    req = HsEntityAttendBackwardRequest(qkv.data_ptr(), None if key_mask is None else key_mask.data_ptr(), grad_out.data_ptr(), n, E,
                                        _DTYPES[_name(qkv.dtype)], _DTYPES[_name(grad_out.dtype)], ptr("grad_qkv"))
    return res, req


def compute(sim, qkv, key_mask=None, stream=None, **kw):
    """HideAndSeekSimulator.attend_entities."""
    res, req = request(sim.gpu_id, qkv, key_mask, **kw)
    _run(sim, "hs_entity_attend", req, stream)
    return res


def compute_backward(sim, qkv, key_mask, grad_out, stream=None, **kw):
    """HideAndSeekSimulator.attend_entities_backward."""
    res, req = request_backward(sim.gpu_id, qkv, key_mask, grad_out, **kw)
    _run(sim, "hs_entity_attend_backward", req, stream)
    return res


def compute_sharded(ssim, qkv, key_mask=None, stream=None, out=True, **kw):
    """ShardedSimulator.attend_entities: every shard works its own rows on its own device."""
    return _shard_calls(ssim, "hs_entity_attend", request, stream, dict(qkv=qkv), None, dict(key_mask=key_mask, out=out), kw)


def compute_backward_sharded(ssim, qkv, key_mask, grad_out, stream=None, grad_qkv=True, **kw):
    """ShardedSimulator.attend_entities_backward: as compute_sharded."""
    return _shard_calls(ssim, "hs_entity_attend_backward", request_backward, stream, dict(qkv=qkv, grad_out=grad_out), None,
                        dict(key_mask=key_mask, grad_qkv=grad_qkv), kw)


# ---- the autograd face ----
def _aligned(t):
    """t, contiguous and ALIGN-byte aligned: itself where it already is, else a copy."""
    t = t.contiguous()
    return t.clone() if t.data_ptr() % ALIGN else t


@functools.lru_cache(maxsize=None)
def _function():
    import torch

    class _Attend(torch.autograd.Function):
        @staticmethod
        def forward(ctx, qkv, key_mask, sim):
            qkv = _aligned(qkv.detach())
            ctx.save_for_backward(qkv, key_mask)
            ctx.sim = sim
            return compute(sim, qkv, key_mask)["out"]

        @staticmethod
        def backward(ctx, grad_out):
            qkv, key_mask = ctx.saved_tensors
            g = compute_backward(ctx.sim, qkv, key_mask, _aligned(grad_out))["grad_qkv"]
            return g.to(qkv.dtype), None, None
    return _Attend


def attend(sim, qkv, key_mask=None, fused=True):
    """out [n, 17, E] of qkv [n, 17, 3, 4, D] as part of the autograd graph: the kernels on `sim`'s device, or with
    fused=False eager() (then `sim` is not used and may be None).  The gradient goes to qkv alone."""
    if fused:
        return _function().apply(qkv, key_mask, sim)
    return eager(qkv, key_mask).to(qkv.dtype)


def _after_gemm(layer, sim, z):
    """What an mlp.DenseNormAct does after its GEMM, on a z computed here (the residual's x + a W_o)."""
    if layer.fused:
        return mlp._function().apply(z, layer.params, sim, layer.eps, layer.slope)
    return mlp.eager(z, layer.params, layer.eps, layer.slope).to(z.dtype)


class AttentionEncoder(_module_base()):
    """The network as a torch module.  Composition only: it makes no kernel call of its own.  forward(sim, rows [n, 296],
    dtype, masked) -> features [n, out] in `dtype`:
      tokens    per table of policy_inputs.TABLES an mlp.DenseNormAct(K, E) on the [n count, K] entities (weight [K, E]
                orthogonal with gain sqrt(2) as SimpleNet.embed's, then bias, LayerNorm and leaky ReLU in k_dense),
                concatenated to x [n, 17, E];
      mask      with masked=True (the actor's rows, whose tables k_pack has multiplied by their visibility masks after
                normalising) key_mask = any(entity's features != 0), self always 1; with masked=False (the critic's) None;
      attend    qkv = x w_qkv + b_qkv, a = attend(qkv, key_mask);
      residual  y = LayerNorm(x + a W_o + b_o): an mlp.DenseNormAct(E, E, slope=1) after its GEMM (a slope of 1 is the
                identity, exactly);
      pool      the mean of y over the valid tokens, in torch;
      out       an mlp.DenseNormAct(E, out) on the pooled row.
    w_qkv and W_o are orthogonal with gain 1 and b_qkv is 0: the project's choices.  With fused=False every piece runs its
    eager() on the same parameters.  Rows beyond what one hs_dense_norm_act call can index (INDEX_LIMIT) are worked in
    pieces and the features concatenated."""

    def __init__(self, embed=128, out=256, heads=HEADS, fused=True, generator=None):
        import torch
        super().__init__()
        if heads != HEADS:
            raise ValueError(f"heads must be {HEADS}, got {heads}")
        if embed not in EMBED_DIMS:
            raise ValueError(f"embed must be one of {EMBED_DIMS}, got {embed}")
        self.embed, self.out, self.heads = embed, out, heads
        self.tokens = torch.nn.ModuleDict({name: mlp.DenseNormAct(K, embed, fused=fused, generator=generator) for name, _, _, K in table_tokens()})
        self.w_qkv = torch.nn.Parameter(torch.empty(embed, 3 * embed))
        self.b_qkv = torch.nn.Parameter(torch.zeros(3 * embed))
        self.residual = mlp.DenseNormAct(embed, embed, slope=1.0, fused=fused, generator=generator)
        self.project = mlp.DenseNormAct(embed, out, fused=fused, generator=generator)
        with torch.no_grad():
            for layer in self.tokens.values():
                torch.nn.init.orthogonal_(layer.weight, gain=math.sqrt(2.0), generator=generator)
            torch.nn.init.orthogonal_(self.w_qkv, generator=generator)
            torch.nn.init.orthogonal_(self.residual.weight, generator=generator)

    @property
    def fused(self):
        return self.project.fused

    @fused.setter
    def fused(self, value):
        for layer in (*self.tokens.values(), self.residual, self.project):
            layer.fused = bool(value)

    def key_mask(self, rows):
        """uint8 [n, 17]: 1 where the entity's features in rows [n, 296] are not all zero, and for self."""
        import torch
        parts = []
        for name, _, count, K in table_tokens():
            lo, hi, _ = TABLES[name]
            t = rows[:, lo:hi].reshape(rows.shape[0], count, K)
            parts.append(torch.ones_like(t[:, :, 0], dtype=torch.bool) if name == "self" else (t != 0).any(-1))
        return torch.cat(parts, 1).to(torch.uint8)

    def forward(self, sim, rows, dtype=None, masked=False):
        import torch
        dtype = rows.dtype if dtype is None else dtype
        n, E = rows.shape[0], self.embed
        most = (INDEX_LIMIT - 1) // (TOKENS * E)                              # rows whose [n 17, E] tokens one k_dense call can index
        if n > most:                                                          # a minibatch pass of 1.92 M rows at E = 128: two pieces
            return torch.cat([self.forward(sim, rows[lo:lo + most], dtype, masked) for lo in range(0, n, most)])
        rows = rows.to(dtype)
        xs = []
        for name, _, count, K in table_tokens():
            lo, hi, _ = TABLES[name]
            xs.append(self.tokens[name](sim, rows[:, lo:hi].reshape(n * count, K)).reshape(n, count, E))
        x = torch.cat(xs, 1)                                                  # [n, 17, E]
        mask = self.key_mask(rows) if masked else None
        qkv = torch.nn.functional.linear(x, self.w_qkv.to(dtype).t(), self.b_qkv.to(dtype)).reshape(n, TOKENS, 3, self.heads, E // self.heads)
        a = attend(sim, qkv, mask, self.fused)
        z = x + a @ self.residual.weight.to(dtype)
        y = _after_gemm(self.residual, sim, z.reshape(n * TOKENS, E)).reshape(n, TOKENS, E)
        if mask is None:
            pooled = y.mean(1)
        else:
            w = mask.to(dtype).unsqueeze(-1)
            pooled = (y * w).sum(1) / w.sum(1)
        return self.project(sim, pooled)
