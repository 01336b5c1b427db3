"""What the learner modules share on the way to a request entry point of libhideseek (include/hideseek.h): the dtype
codes, the checks of tensors handed in, and the two ways of calling — one handle, blocking or on a stream, and one
request per shard on side streams.  Internal: imported by the package's public modules."""
import ctypes as C

_DTYPES = {"float32": 1, "bfloat16": 3, "float16": 4}      # HS_DTYPE_F32 / _BF16 / _F16


def _name(dtype):
    return str(dtype).replace("torch.", "")


def stream_handle(stream):
    """The raw hipStream_t of a torch.cuda.Stream (or the integer itself)."""
    return int(getattr(stream, "cuda_stream", stream))


# ---- tensors handed in ----
def _rows(name, t, n, L, dev, what):
    """Check a [n, W >= L] tensor that is contiguous in its last dimension (logits, grad_logits)."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor")
    what = f"{name} must be a {' / '.join(_DTYPES)} tensor of shape ({what}, W >= {L}), contiguous in its last dimension, on {dev}"
    if t.dim() != 2 or t.shape[0] < 1 or (n is not None and t.shape[0] != n) or t.shape[1] < L:
        raise ValueError(f"{what}: its shape is {tuple(t.shape)}")
    if _name(t.dtype) not in _DTYPES:
        raise ValueError(f"{what}: its dtype is {t.dtype}")
    stride = max(int(t.stride(0)), L) if t.shape[0] > 1 else max(int(t.shape[1]), L)
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < L) or t.shape[0] * stride >= 2 ** 31:
        raise ValueError(f"{what}: its stride is {tuple(t.stride())} (n * stride must stay below 2^31)")
    return stride


def _vector(name, t, n, dev, dtypes, tail=()):
    """Check a contiguous per-sample tensor [n] + tail (or [n, 1] when tail is empty)."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor")
    shape = (n,) + tail
    what = f"{name} must be a contiguous {' / '.join(dtypes)} tensor of shape {shape} on {dev}"
    if tuple(t.shape) != shape and not (not tail and tuple(t.shape) == (n, 1)):
        raise ValueError(f"{what}: its shape is {tuple(t.shape)}")
    if _name(t.dtype) not in dtypes:
        raise ValueError(f"{what}: its dtype is {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: it is not contiguous")


def _given(name, t, shape, dtypes, dev):
    """Check a contiguous tensor of exactly `shape` that the caller handed in for an output (or a fixed-shape input)."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be True, None or a torch tensor")
    what = f"{name} must be a contiguous {' / '.join(dtypes)} tensor of shape {shape} on {dev}"
    if tuple(t.shape) != shape:
        raise ValueError(f"{what}: its shape is {tuple(t.shape)}")
    if _name(t.dtype) not in dtypes:
        raise ValueError(f"{what}: its dtype is {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: it is not contiguous")


def _overlap(a, b):
    """Whether the storage ranges of two tensors intersect."""
    def span(t):
        last = sum((s - 1) * st for s, st in zip(t.shape, t.stride()))
        return t.data_ptr(), t.data_ptr() + (last + 1) * t.element_size()
    (a0, a1), (b0, b1) = span(a), span(b)
    return a0 < b1 and b0 < a1


def _disjoint(outputs, inputs, dev):
    """No output [(name, tensor)] overlaps an input or an earlier output, and then all of them are on `dev`: shapes,
    dtypes and strides have been checked first, so that every one of them is reported whatever device the tensors are on."""
    for k, t in outputs:
        for k2, t2 in inputs:
            if _overlap(t, t2):
                raise ValueError(f"{k} overlaps {k2}")
    for i, (k, t) in enumerate(outputs):
        for k2, t2 in outputs[:i]:
            if _overlap(t, t2):
                raise ValueError(f"{k} overlaps {k2}")
    for k, t in inputs + outputs:
        if t.device != dev:
            raise ValueError(f"{k} must be on {dev}: it is on {t.device}")


# ---- one entry per shard ----
def _per_shard(ssim, name, arg):
    n = len(ssim.shards)
    if arg is None or arg is True or arg is False:
        return [arg] * n
    if len(arg) != n:
        raise ValueError(f"{name}: one entry per shard ({n}) expected")
    return list(arg)


def _shard_list(ssim, name, arg):
    import torch
    if isinstance(arg, torch.Tensor) or arg is None or len(arg) != len(ssim.shards):
        raise ValueError(f"{name}: one tensor per shard ({len(ssim.shards)}) expected")
    return list(arg)


def _shard_params(ssim, params):
    import torch
    return [params] * len(ssim.shards) if isinstance(params, torch.Tensor) else _per_shard(ssim, "params", params)


# ---- the calls ----
_enqueue = [0]              # depth of on_current_stream() contexts


class on_current_stream:
    """Inside this context a call given stream=None is enqueued on torch's current stream of the handle's device without
    waiting, where it would otherwise block: the module faces (EntityEncoder, MLP, LSTMCore and their backward) pass no
    stream, and the update loop (gpu_hideseek.trainer) runs them here so that nothing in it waits for the device."""

    def __enter__(self):
        _enqueue[0] += 1
        return self

    def __exit__(self, *exc):
        _enqueue[0] -= 1
        return False


def _run(sim, fn, req, stream, *extra):
    """Entry point `fn` of `sim`'s handle with request `req` (and what follows it in the signature): blocking with
    stream=None (outside on_current_stream()), else `fn`_async on the torch.cuda.Stream or raw handle, without
    synchronising."""
    from ._native import check
    if stream is None and _enqueue[0]:
        import torch
        stream = torch.cuda.current_stream(sim.gpu_id)
    if stream is None:
        check(getattr(sim._L, fn)(sim._h, C.byref(req), *extra))
    else:
        check(getattr(sim._L, fn + "_async")(sim._h, C.c_void_p(stream_handle(stream)), C.byref(req), *extra))


def _sharded(ssim, fn, make, stream):
    """make(i, shard) -> (result, request) for every shard, then entry point `fn` (a name for _run, or a callable
    (shard, request, stream)) for each on the shard's entry of `stream`; with None there, on a side stream of its device
    ordered after that device's current stream, all of which are waited for once every call is enqueued.  Returns the
    list of the shards' results."""
    import torch
    streams = _per_shard(ssim, "stream", stream)
    reqs = [make(i, s) for i, s in enumerate(ssim.shards)]
    waits = []
    for s, (res, req), st in zip(ssim.shards, reqs, streams):
        if st is None:
            st = torch.cuda.Stream(device=s.gpu_id)
            st.wait_stream(torch.cuda.current_stream(s.gpu_id))
            waits.append(st)
        if callable(fn):
            fn(s, req, st)
        else:
            _run(s, fn, req, st)
    for st in waits:
        st.synchronize()
    return [res for res, _ in reqs]
