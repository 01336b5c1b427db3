"""What can be checked of grouped advantages (include/hideseek.h: hs_compute_gae_grouped; advantages.request(groups=G))
without a GPU: the header and its ctypes mirror, the exported symbols, how the grid is cut against the workspace the handle
allocates, and the refusals that come before any device is looked at."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLDS, AGENTS, T = 36, 6, 8
R = WORLDS * AGENTS


def test_header_mirror_and_symbols_agree(hideseek_lib):
    from gpu_hideseek import advantages as A, league
    src = open(os.path.join(ROOT, "include", "hideseek.h")).read()
    flat = " ".join(src.split())
    assert "int32_t hs_compute_gae_grouped(hs_sim *sim, const hs_gae_grouped_request *req);" in flat
    assert "int32_t hs_compute_gae_grouped_async(hs_sim *sim, void *hip_stream, const hs_gae_grouped_request *req);" in flat
    body = re.search(r"typedef struct hs_gae_grouped_request \{(.*?)\} hs_gae_grouped_request;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in A.HsGaeGroupedRequest._fields_] == ["gae", "groups", "reserved"]
    # hs_gae_request keeps its layout, and the grouped request starts with it
    assert C.sizeof(A.HsGaeRequest) == 80 and A.HsGaeRequest.moments.offset == 72
    assert C.sizeof(A.HsGaeGroupedRequest) == 88 and A.HsGaeGroupedRequest.gae.offset == 0 and A.HsGaeGroupedRequest.groups.offset == 80
    assert A.MAX_GROUPS == league.MAX_POLICIES == int(re.search(r"HS_LEAGUE_MAX_POLICIES = (\d+)", src).group(1))
    lib = C.CDLL(hideseek_lib)
    assert hasattr(lib, "hs_compute_gae_grouped") and hasattr(lib, "hs_compute_gae_grouped_async")
    csrc = os.path.join(ROOT, "marl-hideandseek_amd", "csrc")
    host, kernel = (open(os.path.join(csrc, f)).read() for f in ("hideseek.hip", "hs_k_gae.h"))
    assert "sizeof(hs_gae_grouped_request) == 88" in host and "offsetof(hs_gae_grouped_request, groups) == 80" in host
    assert "sizeof(hs_gae_request) == 80" in host
    grouped = kernel[kernel.index("void k_gae_grouped("):]
    assert grouped.count("gae_row<T, ") == 8 and "atomic" not in re.sub(r"//.*", "", kernel)
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"hs_compute_gae_grouped", "hs_compute_gae_grouped_async"' in entry


def test_the_grid_never_needs_more_workspace_rows_than_the_handle_allocates():
    """gae_grid (csrc/hs_k_gae.h) restated: G groups of gae_grid(R / G) workgroups each write one row of partials; the
    handle allocates gae_grid(R) + 16 rows.  With one group the grid is hs_compute_gae's own."""
    def grid(rows):
        return (rows + 63) // 64
    for g in range(1, 17):
        for m in (1, 36, 63, 64, 65, 108, 6000, 10 ** 6 + 1):
            assert g * grid(m) <= grid(g * m) + 16, (g, m)
    assert grid(216) == 4 and [grid(216 // g) for g in (1, 2, 3, 6)] == [4, 2, 2, 1]


def test_request_refuses_before_any_device_is_looked_at():
    import torch
    from gpu_hideseek import advantages as A
    x = dict(rewards=torch.zeros(T, R), dones=torch.zeros(T, R, dtype=torch.int32), values=torch.zeros(T, R), bootstrap=torch.zeros(R))

    def call(**kw):
        args = dict(x, groups=3)
        args.update(kw)
        return A.request(WORLDS, AGENTS, 0, **args)

    f64 = torch.float64
    cases = [
        (dict(groups=0), "groups must be"), (dict(groups=17), "groups must be"), (dict(groups=2.0), "groups must be"), (dict(groups=True), "groups must be"),
        (dict(groups=5), "multiple of groups"), (dict(groups=16), "multiple of groups"),
        (dict(moments=torch.zeros(5, dtype=f64)), "moments.*shape"), (dict(moments=torch.zeros(2, 5, dtype=f64)), "moments.*shape"),
        (dict(moments=torch.zeros(3, 5)), "moments.*dtype"), (dict(moments=torch.zeros(3, 10, dtype=f64)[:, ::2]), "moments.*not contiguous"),
        (dict(groups=1, moments=torch.zeros(5, dtype=f64)), "moments.*shape"),
        (dict(gamma=1.5), "gamma"), (dict(rewards=torch.zeros(T, R - 1)), "rewards.*shape"),
        (dict(advantages=None, returns=None), "nothing to do"),
        # well formed: the device comes last
        (dict(moments=torch.zeros(3, 5, dtype=f64)), "it is on cpu"),
    ]
    for kw, what in cases:
        with pytest.raises(ValueError, match=what):
            call(**kw)
    # groups=None is the plain request, unchanged
    with pytest.raises(ValueError, match="moments.*shape"):
        call(groups=None, moments=torch.zeros(3, 5, dtype=f64))
    with pytest.raises(ValueError, match="it is on cpu"):
        call(groups=None, moments=torch.zeros(5, dtype=f64))
