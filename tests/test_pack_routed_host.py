"""What can be checked of the routed pack (include/hideseek.h: hs_pack_policy_inputs_routed; policy_inputs.request_routed,
ObsNormaliser(table=...)) without a GPU: the header and its ctypes mirror, the exported symbols, how the kernel header cuts
its grid, and the refusals that come before any device is looked at."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW, MOMENTS, TABLE = 296, 593, 592


class _Sim:
    num_worlds, agents_per_world, gpu_id = 18, 6, 0


def test_header_mirror_and_symbols_agree(hideseek_lib):
    from gpu_hideseek import league, policy_inputs as P
    src = open(os.path.join(ROOT, "include", "hideseek.h")).read()
    flat = " ".join(src.split())
    assert "int32_t hs_pack_policy_inputs_routed(hs_sim *sim, const hs_pack_routed_request *req);" in flat
    assert "int32_t hs_pack_policy_inputs_routed_async(hs_sim *sim, void *hip_stream, const hs_pack_routed_request *req);" in flat
    body = re.search(r"typedef struct hs_pack_routed_request \{(.*?)\} hs_pack_routed_request;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in P.HsPackRoutedRequest._fields_]
    want = dict(actor=0, actor_dtype=8, critic=16, critic_dtype=24, row_of_slot=32, num_policies=40, tables=48, moments=56, moments_stride=64, bad=72)
    assert C.sizeof(P.HsPackRoutedRequest) == 80
    assert {n: getattr(P.HsPackRoutedRequest, n).offset for n in want} == want
    assert list(want) == names
    assert P.MAX_POLICIES == league.MAX_POLICIES == int(re.search(r"HS_LEAGUE_MAX_POLICIES = (\d+)", src).group(1))
    assert (P.ROW, P.MOMENTS, P.NORM_TABLE) == (ROW, MOMENTS, TABLE)
    L = C.CDLL(hideseek_lib)
    assert hasattr(L, "hs_pack_policy_inputs_routed") and hasattr(L, "hs_pack_policy_inputs_routed_async")
    # the host section checks the same layout, and the kernel reuses pack_blocks instead of a copy of it
    csrc = os.path.join(ROOT, "marl-hideandseek_amd", "csrc")
    host, kernel = (open(os.path.join(csrc, f)).read() for f in ("hideseek.hip", "hs_k_pack_routed.h"))
    assert "sizeof(hs_pack_routed_request) == 80" in host and "offsetof(hs_pack_routed_request, bad) == 72" in host
    assert "pack_blocks<TA, TC, MOM, NORM>(" in kernel and "pack_write" not in re.sub(r"//.*", "", kernel)
    assert len(re.findall(r"__global__", kernel)) == len(re.findall(r"template <typename TA, typename TC, bool MOM, bool NORM>\n__global__", kernel)) == 1


def test_the_grid_never_needs_more_workspace_rows_than_the_handle_allocates():
    """pack_routed_grid (csrc/hs_k_pack_routed.h) restated: G workgroups per policy, N G rows of workspace; the handle
    allocates min(1024, R / 32 + 16) rows.  With one policy the grid is hs_pack_policy_inputs' own."""
    def grid(per_policy, n):
        return min((per_policy + 31) // 32, 1024 // n)
    for n in range(1, 17):
        for rows in (n, 36 * n, 1024 * n, 32 * 1024 + n, 12288 * n, 10 ** 6 * n):
            g = grid(rows // n, n)
            assert 1 <= g and n * g <= min(1024, rows // 32 + 16), (n, rows, g)
    assert [grid(r, 1) for r in (1, 32, 33, 32768, 32769, 10 ** 6)] == [1, 1, 2, 1024, 1024, 1024]


def test_request_routed_refuses_before_any_device_is_looked_at():
    import torch
    from gpu_hideseek import policy_inputs as P
    R, N = _Sim.num_worlds * _Sim.agents_per_world, 3
    ros = torch.arange(R, dtype=torch.int32)
    tables = torch.zeros(N, TABLE)
    raw = torch.zeros(N * TABLE + 8)
    off = next(o for o in range(1, 5) if raw[o:].data_ptr() % 16)

    def call(**kw):
        args = dict(row_of_slot=ros, num_policies=N, actor=torch.zeros(R, ROW), tables=tables)
        args.update(kw)
        return P.pack_routed(_Sim(), args.pop("row_of_slot"), args.pop("num_policies"), **args)

    cases = [
        (dict(num_policies=0), "num_policies"), (dict(num_policies=17), "num_policies"), (dict(num_policies=2.0), "num_policies"),
        (dict(num_policies=True), "num_policies"), (dict(num_policies=5), "multiple of num_policies"), (dict(num_policies=16), "multiple of num_policies"),
        (dict(row_of_slot=ros[:-1]), "row_of_slot.*shape"), (dict(row_of_slot=ros.long()), "row_of_slot.*dtype"), (dict(row_of_slot=ros.tolist()), "row_of_slot must be"),
        (dict(row_of_slot=torch.arange(2 * R, dtype=torch.int32)[::2]), "row_of_slot.*not contiguous"),
        (dict(tables=tables[:2]), "tables.*shape"), (dict(tables=torch.zeros(N * TABLE)), "tables.*shape"), (dict(tables=tables.double()), "tables.*dtype"),
        (dict(tables=raw[off:off + N * TABLE].view(N, TABLE)), "tables must be 16-byte aligned"), (dict(tables=[0.0] * TABLE), "tables must be"),
        (dict(bad=torch.zeros(2, dtype=torch.int32)), "bad.*shape"), (dict(bad=torch.zeros(1)), "bad.*dtype"), (dict(bad=0), "bad must be"),
        (dict(actor=torch.zeros(R - 1, ROW)), "actor.*shape"), (dict(actor=torch.zeros(R, ROW, dtype=torch.float64)), "actor.*dtype"),
        (dict(actor=None, critic=torch.zeros(R, 2 * ROW)[:, ::2]), "critic.*not contiguous"), (dict(actor="rows"), "actor must be"),
        (dict(actor=None, moments=torch.zeros(N, MOMENTS)), "moments.*dtype"), (dict(actor=None, moments=torch.zeros(MOMENTS, dtype=torch.float64)), "moments.*shape"),
        (dict(actor=None, moments=torch.zeros(N, 2 * MOMENTS, dtype=torch.float64)[:, ::2]), "moments.*stride"), (dict(actor=None, moments=[0.0]), "moments must be"),
        (dict(actor=None), "no output requested"),
        # well formed: the device comes last
        (dict(), "actor must be.*it is on cpu"), (dict(actor=None, moments=torch.zeros(N, MOMENTS, dtype=torch.float64)), "moments must be.*it is on cpu"),
    ]
    for kw, what in cases:
        with pytest.raises(ValueError, match=what):
            call(**kw)


def test_a_normaliser_refuses_a_table_it_cannot_keep():
    import torch
    from gpu_hideseek import policy_inputs as P
    for table, what in ((torch.zeros(TABLE - 1), "shape"), (torch.zeros(2, TABLE), "shape"), (torch.zeros(TABLE, dtype=torch.float64), "dtype"),
                        (torch.zeros(2 * TABLE)[::2], "not contiguous"), ([0.0] * TABLE, "normaliser must be"), (torch.zeros(TABLE), "it is on cpu")):
        with pytest.raises(ValueError, match=what):
            P.ObsNormaliser(0, table=table)
    with pytest.raises(ValueError, match="decay"):
        P.ObsNormaliser(0, decay=1.0, table=torch.zeros(TABLE))
