"""What can be checked of the routed sampler (include/hideseek.h: hs_sample_actions_routed; action_sampling.request_routed)
without a GPU: the header and its ctypes mirror, the exported symbols, that the kernel reuses k_sample's head and image,
and the refusals that come before any device is looked at."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 19


class _Sim:
    num_worlds, agents_per_world, gpu_id = 36, 6, 0


def test_header_mirror_and_symbols_agree(hideseek_lib):
    from gpu_hideseek import action_sampling as A
    src = open(os.path.join(ROOT, "include", "hideseek.h")).read()
    flat = " ".join(src.split())
    assert "int32_t hs_sample_actions_routed(hs_sim *sim, const hs_sample_routed_request *req);" in flat
    assert "int32_t hs_sample_actions_routed_async(hs_sim *sim, void *hip_stream, const hs_sample_routed_request *req);" in flat
    body = re.search(r"typedef struct hs_sample_routed_request \{(.*?)\} hs_sample_routed_request;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    body = re.sub(r"\[\w+\]", "", body)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in A.HsSampleRoutedRequest._fields_]
    want = dict(logits=0, logits_dtype=8, logits_stride=12, buckets=16, mode=36, flags=40, seed=44, counter=52, row_of_slot=56, action_rows=64, action=72,
                log_prob=80, entropy=88, head_log_prob=96, bad=104)
    assert C.sizeof(A.HsSampleRoutedRequest) == 112
    assert {n: getattr(A.HsSampleRoutedRequest, n).offset for n in want} == want
    assert list(want) == names
    # the plain request's prefix is this request's prefix: the two share their first nine fields
    assert [(f[0], getattr(A.HsSampleRequest, f[0]).offset) for f in A.HsSampleRequest._fields_[:8]] == \
           [(f[0], getattr(A.HsSampleRoutedRequest, f[0]).offset) for f in A.HsSampleRoutedRequest._fields_[:8]]
    lib = C.CDLL(hideseek_lib)
    assert hasattr(lib, "hs_sample_actions_routed") and hasattr(lib, "hs_sample_actions_routed_async")
    csrc = os.path.join(ROOT, "marl-hideandseek_amd", "csrc")
    host, kernel = (open(os.path.join(csrc, f)).read() for f in ("hideseek.hip", "hs_k_sample_routed.h"))
    assert "sizeof(hs_sample_routed_request) == 112" in host and "offsetof(hs_sample_routed_request, bad) == 104" in host
    code = re.sub(r"//.*", "", kernel)
    assert '#include "hs_k_sample.h"' in kernel and "sample_head(" in code and "SampleImage im" in code
    assert "HSD void sample_head" not in code and "struct SampleImage" not in code          # reused, not copied
    assert len(re.findall(r"__global__", code)) == 1 and "atomicAdd(ra.bad, 1)" in code
    assert len(re.findall(r"atomic", code)) == 1                                              # the integer count alone
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"hs_sample_actions_routed", "hs_sample_actions_routed_async"' in entry


def test_request_routed_refuses_before_any_device_is_looked_at():
    import torch
    from gpu_hideseek import action_sampling as A
    R = _Sim.num_worlds * _Sim.agents_per_world
    ros = torch.arange(R, dtype=torch.int32)
    logits = torch.zeros(R, L)

    def call(**kw):
        args = dict(logits=logits, row_of_slot=ros)
        args.update(kw)
        return A.sample_routed(_Sim(), args.pop("logits"), args.pop("row_of_slot"), **args)

    i32 = torch.int32
    cases = [
        (dict(mode="evaluate"), "mode must be one of draw, greedy"), (dict(mode="sample"), "mode must be"), (dict(mode=2), "mode must be"),
        (dict(flags=1), "flags must be 0"), (dict(flags=True), "flags must be 0"),
        (dict(buckets=(5, 5, 5, 2)), "buckets"), (dict(buckets=(17, 1, 1, 1, 1)), "buckets"), (dict(buckets=(16, 16, 16, 16, 1)), "more than 64"),
        (dict(seed=(1,)), "seed"),
        (dict(logits=logits[:-1]), "logits.*shape"), (dict(logits=torch.zeros(R, L - 1)), "logits.*shape"), (dict(logits=logits.double()), "logits.*dtype"),
        (dict(logits=torch.zeros(R, 2 * L)[:, ::2]), "logits.*stride"), (dict(logits=logits.tolist()), "logits must be"),
        (dict(row_of_slot=None), "row_of_slot must be"), (dict(row_of_slot=ros[:-1]), "row_of_slot.*shape"), (dict(row_of_slot=ros.long()), "row_of_slot.*dtype"),
        (dict(row_of_slot=torch.arange(2 * R, dtype=i32)[::2]), "row_of_slot.*not contiguous"),
        (dict(action_rows=torch.zeros(R, 5, dtype=i32)), "nothing to do"), (dict(action_rows=torch.zeros(R, 4, dtype=i32), log_prob=True), "action_rows.*shape"),
        (dict(action_rows=torch.zeros(R, 5), log_prob=True), "action_rows.*dtype"), (dict(action_rows=True, log_prob=True), "action_rows must be"),
        (dict(action=torch.zeros(R, 5)), "action.*dtype"), (dict(action=torch.zeros(R - 1, 5, dtype=i32)), "action.*shape"),
        (dict(log_prob=torch.zeros(R, 2)), "log_prob.*shape"), (dict(entropy=torch.zeros(2 * R)[::2]), "entropy.*not contiguous"),
        (dict(head_log_prob=torch.zeros(R, 5, dtype=torch.float64)), "head_log_prob.*dtype"), (dict(log_prob="yes"), "log_prob must be"),
        (dict(bad=torch.zeros(2, dtype=i32)), "bad.*shape"), (dict(bad=torch.zeros(1)), "bad.*dtype"), (dict(bad=0), "bad must be"),
        # well formed: the device comes last
        (dict(), "logits must be on.*it is on cpu"), (dict(log_prob=torch.zeros(R)), "it is on cpu"),
    ]
    for kw, what in cases:
        with pytest.raises(ValueError, match=what):
            call(**kw)
    # overlaps are told before the device
    act = torch.zeros(R, 5, dtype=i32)
    with pytest.raises(ValueError, match="action overlaps action_rows"):
        call(action_rows=act, action=act)
    with pytest.raises(ValueError, match="action_rows overlaps row_of_slot"):
        call(row_of_slot=act.view(-1)[:R], action_rows=act, log_prob=True)
    both = torch.zeros(2 * R)
    with pytest.raises(ValueError, match="entropy overlaps log_prob"):
        call(log_prob=both[:R], entropy=both[R - 1:2 * R - 1])
