"""The entity encoder: the first layer of the reference's SimpleNet (scripts/jax_policy.py:113-161) over packed
policy-input rows, forward and parameter gradient each by one kernel (hs_entity_encode, hs_entity_encode_backward,
csrc/hs_k_embed.h).

Every entity of the four tables of a row (policy_inputs.TABLES: self [45], agents [5, 14], boxes [9, 17], ramps [2, 14])
goes through its table's Dense(E), a LayerNorm and a leaky ReLU; agents, boxes and ramps are max-pooled over their
entities; the results are concatenated into [rows, 4 E].  include/hideseek.h states the arithmetic, IEEE f32 in a fixed
order.  Actor and critic run it on their rows in every rollout step and every minibatch:

    enc = entity_encoder.EntityEncoder(64).cuda()                    # one flat float32 Parameter of 102 * 64 elements
    sim.pack_policy_inputs(actor=actor_rows[t], critic=critic_rows[t])
    feats = enc(sim, actor_rows[t])                                  # [rows, 256], part of the autograd graph
    loss = head(feats) ...; loss.backward(); optimiser.step()        # the backward kernel hands grad_params to autograd

or without autograd, into a rollout buffer:

    sim.encode_entities(actor_rows[t], enc.params.detach(), features=feat_buf[t])

No gradient with respect to the rows is computed: observations are leaves and the normaliser is not trained by gradient.
A tie of the max-pool goes to the first entity (JAX splits it evenly); entities tie in practice because their inputs are
identical (the actor's masked-out entities are all-zero rows), and then every parameter's gradient is the same either
way.  eager() is the same composition in plain torch, for readers, tools/embed_bench.py and the tests.
"""
import ctypes as C
import functools
import math

from ._request import _DTYPES, _above_zero, _dtype_arg, _finite, _module_base, _name, _one_of, _outputs, _run, _shard_calls, _tensor, _wanted
from .policy_inputs import ROW, TABLES

EMBED_DIMS = (32, 64, 128)
PARAM_ROWS = 102          # HS_EMBED_PARAM_ROWS: the sum over the tables of K + 3
MAX_GRID_BWD = 512        # HS_EMBED_MAX_GRID_BWD: workgroups (and workspace slices) of a backward call at the most
SUM_SEGS = 8              # HS_EMBED_SUM_SEGS
WAVES = 4                 # waves of a workgroup
DEFAULT_EPS, DEFAULT_SLOPE = 1e-6, 0.01      # flax's LayerNorm epsilon and leaky_relu negative_slope
POOLED = tuple(TABLES)[1:]                   # the max-pooled tables, in the order of argmax's second axis


def rows_per_block(E):
    """R: the rows a workgroup takes per round (HS_EMBED_ROWS_PER_WAVE(E) * 4)."""
    return WAVES * (2 if E == 32 else 1)


class HsEntityEncodeRequest(C.Structure):
    """hs_entity_encode_request (include/hideseek.h)."""
    _fields_ = [("rows", C.c_void_p), ("params", C.c_void_p), ("n", C.c_int32), ("rows_dtype", C.c_int32), ("embed_dim", C.c_int32),
                ("features_dtype", C.c_int32), ("eps", C.c_float), ("slope", C.c_float), ("features", C.c_void_p), ("argmax", C.c_void_p)]


class HsEntityEncodeBackwardRequest(C.Structure):
    """hs_entity_encode_backward_request (include/hideseek.h)."""
    _fields_ = [("rows", C.c_void_p), ("params", C.c_void_p), ("grad_features", C.c_void_p), ("argmax", C.c_void_p), ("n", C.c_int32),
                ("rows_dtype", C.c_int32), ("embed_dim", C.c_int32), ("grad_dtype", C.c_int32), ("eps", C.c_float), ("slope", C.c_float),
                ("grad_params", C.c_void_p)]


# ---- the parameters: one description, from policy_inputs.TABLES ----
def _embed_dim(E):
    return _one_of("embed_dim", E, EMBED_DIMS)


def param_layout(E):
    """{table: {"kernel": (first, one past the last, (K, E)), "bias": (.., (E,)), "scale": .., "shift": ..}}: the element
    ranges of the flat parameter tensor of PARAM_ROWS * E float32, in order: for each table of policy_inputs.TABLES the
    Dense kernel W [K, E] (in-features major), its bias, and the LayerNorm's scale (gamma) and shift (beta)."""
    E = _embed_dim(E)
    out, at = {}, 0
    for name, (_, _, shape) in TABLES.items():
        K = shape[-1]
        out[name] = {}
        for part, sh in (("kernel", (K, E)), ("bias", (E,)), ("scale", (E,)), ("shift", (E,))):
            size = math.prod(sh)
            out[name][part] = (at, at + size, sh)
            at += size
    assert at == PARAM_ROWS * E
    return out


def views(params, E):
    """The named zero-copy views of a flat parameter (or gradient) tensor: {table: {part: tensor}} after param_layout."""
    if params.dim() != 1 or params.numel() != PARAM_ROWS * _embed_dim(E):
        raise ValueError(f"params must have shape ({PARAM_ROWS * E},), got {tuple(params.shape)}")
    return {t: {p: params[lo:hi].view(sh) for p, (lo, hi, sh) in parts.items()} for t, parts in param_layout(E).items()}


def init_params(E, generator=None):
    """A fresh flat float32 parameter tensor (on the CPU) as SimpleNet.embed initialises it: kernels orthogonal with gain
    sqrt(2), biases 0, LayerNorm scale 1 and shift 0."""
    import torch
    p = torch.zeros(PARAM_ROWS * _embed_dim(E), dtype=torch.float32)
    for parts in views(p, E).values():
        torch.nn.init.orthogonal_(parts["kernel"], gain=math.sqrt(2.0), generator=generator)
        parts["scale"].fill_(1.0)
    return p


def eager(rows, params, E, eps=DEFAULT_EPS, slope=DEFAULT_SLOPE):
    """The plain-torch composition in the dtype of params (float32, or float64 for a reference): [n, 4 E] features of
    rows [n, 296].  Differentiable in params."""
    import torch
    from .policy_inputs import views as tables
    feats = []
    for name, x in tables(rows.to(params.dtype)).items():
        p = views(params, E)[name]
        y = torch.nn.functional.layer_norm(x @ p["kernel"] + p["bias"], (E,), p["scale"], p["shift"], eps)
        a = torch.nn.functional.leaky_relu(y, slope)
        feats.append(a if name == "self" else a.amax(dim=-2))
    return torch.cat(feats, dim=-1)


# ---- the fused calls ----
def _common(gpu_id, rows, params, embed_dim, eps, slope):
    import torch
    dev = torch.device("cuda", gpu_id)
    E = _embed_dim(embed_dim)
    eps, slope = _finite("eps", eps), _finite("slope", slope)
    _above_zero("eps", eps)
    _tensor("rows", rows, ("n >= 1", ROW), _DTYPES, dev, bound=max(ROW, 4 * E))
    _tensor("params", params, (PARAM_ROWS * E,), ("float32",), dev)
    return dev, E, int(rows.shape[0]), eps, slope


def request(gpu_id, rows, params, embed_dim=64, eps=DEFAULT_EPS, slope=DEFAULT_SLOPE, features=True, argmax=None, dtype=None):
    """Validate a forward call over the n = rows.shape[0] rows on GPU `gpu_id`, allocate the outputs given as True
    (features in `dtype`, by default the dtype of the rows; argmax uint8 [n, 3, E]), and return ({name: tensor},
    HsEntityEncodeRequest).  Raises ValueError before the library is involved."""
    import torch
    dev, E, n, eps, slope = _common(gpu_id, rows, params, embed_dim, eps, slope)
    outputs = _wanted((("features", features), ("argmax", argmax)), "neither features nor argmax requested")
    _dtype_arg("dtype", dtype)
    specs = {"features": ((n, 4 * E), rows.dtype if dtype is None else dtype, _DTYPES), "argmax": ((n, 3, E), torch.uint8)}
    res, ptr = _outputs(outputs, specs, [("rows", rows), ("params", params)], dev)
    req = HsEntityEncodeRequest(rows.data_ptr(), params.data_ptr(), n, _DTYPES[_name(rows.dtype)], E,
                                _DTYPES[_name(res["features"].dtype)] if "features" in res else 0, eps, slope, ptr("features"), ptr("argmax"))
    return res, req


def request_backward(gpu_id, rows, params, grad_features, argmax, embed_dim=64, eps=DEFAULT_EPS, slope=DEFAULT_SLOPE, grad_params=True):
    """Validate a backward call, allocate grad_params when it is True, and return ({"grad_params": tensor},
    HsEntityEncodeBackwardRequest).  Raises ValueError before the library is involved."""
    import torch
    dev, E, n, eps, slope = _common(gpu_id, rows, params, embed_dim, eps, slope)
    if not isinstance(grad_features, torch.Tensor) or not isinstance(argmax, torch.Tensor):
        raise ValueError("grad_features and argmax must be torch tensors")
    _tensor("grad_features", grad_features, (n, 4 * E), _DTYPES, dev)
    _tensor("argmax", argmax, (n, 3, E), ("uint8",), dev)
    inputs = [("rows", rows), ("params", params), ("grad_features", grad_features), ("argmax", argmax)]
    flat = ((PARAM_ROWS * E,), torch.float32, lambda k, t: _tensor(k, t, (PARAM_ROWS * E,), ("float32",), dev))      # the one output: not optional
    res, ptr = _outputs({"grad_params": grad_params}, {"grad_params": flat}, inputs, dev)
    req = HsEntityEncodeBackwardRequest(rows.data_ptr(), params.data_ptr(), grad_features.data_ptr(), argmax.data_ptr(), n,
                                        _DTYPES[_name(rows.dtype)], E, _DTYPES[_name(grad_features.dtype)], eps, slope, ptr("grad_params"))
    return res, req


def compute(sim, rows, params, stream=None, **kw):
    """HideAndSeekSimulator.encode_entities."""
    res, req = request(sim.gpu_id, rows, params, **kw)
    _run(sim, "hs_entity_encode", req, stream)
    return res


def compute_backward(sim, rows, params, grad_features, argmax, stream=None, **kw):
    """HideAndSeekSimulator.encode_entities_backward."""
    res, req = request_backward(sim.gpu_id, rows, params, grad_features, argmax, **kw)
    _run(sim, "hs_entity_encode_backward", req, stream)
    return res


def compute_sharded(ssim, rows, params, stream=None, features=True, argmax=None, **kw):
    """ShardedSimulator.encode_entities: every shard encodes its own rows on its own device."""
    return _shard_calls(ssim, "hs_entity_encode", request, stream, dict(rows=rows), dict(params=params), dict(features=features, argmax=argmax), kw)


def compute_backward_sharded(ssim, rows, params, grad_features, argmax, stream=None, grad_params=True, **kw):
    """ShardedSimulator.encode_entities_backward: as compute_sharded; every shard's grad_params holds the sum over its own
    rows (add them for shared parameters)."""
    return _shard_calls(ssim, "hs_entity_encode_backward", request_backward, stream, dict(rows=rows, grad_features=grad_features, argmax=argmax),
                        dict(params=params), dict(grad_params=grad_params), kw)


# ---- the autograd face ----
@functools.lru_cache(maxsize=None)
def _function():
    import torch

    class _Encode(torch.autograd.Function):
        @staticmethod
        def forward(ctx, params, sim, rows, E, eps, slope, dtype):
            out = compute(sim, rows, params.detach(), embed_dim=E, eps=eps, slope=slope, features=True, argmax=True, dtype=dtype)
            ctx.save_for_backward(params, rows, out["argmax"])
            ctx.call = (sim, E, eps, slope)
            return out["features"]

        @staticmethod
        def backward(ctx, grad):
            params, rows, argmax = ctx.saved_tensors
            sim, E, eps, slope = ctx.call
            g = compute_backward(sim, rows, params.detach(), grad.contiguous(), argmax, embed_dim=E, eps=eps, slope=slope)["grad_params"]
            return g, None, None, None, None, None, None
    return _Encode


class EntityEncoder(_module_base()):
    """The encoder as a torch module: one flat float32 Parameter `params` of PARAM_ROWS * embed_dim elements
    (param_layout; named_views() gives the tables' kernels, biases, scales and shifts as views).  forward(sim, rows) runs
    the forward kernel on `sim`'s device and returns features [n, 4 E] (in `dtype`, by default the rows' dtype) as part
    of the autograd graph of `params`: its backward runs the backward kernel.  rows get no gradient."""

    def __init__(self, embed_dim=64, eps=DEFAULT_EPS, slope=DEFAULT_SLOPE, generator=None):
        import torch
        super().__init__()
        self.embed_dim, self.eps, self.slope = _embed_dim(embed_dim), float(eps), float(slope)
        self.params = torch.nn.Parameter(init_params(embed_dim, generator))

    def named_views(self):
        return views(self.params, self.embed_dim)

    def forward(self, sim, rows, dtype=None):
        return _function().apply(self.params, sim, rows.detach(), self.embed_dim, self.eps, self.slope, dtype)
