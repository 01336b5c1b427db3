"""The contract of hs_episode_stats (include/hideseek.h) restated in numpy, and what can be checked of it without a GPU:
properties of the restatement, the refusals of gpu_hideseek.episodes.request, stats_to_metrics against float64 and the
agreement of the ctypes mirror with the header.  tests/test_gpu_episodes.py compares the kernel with episode_step bit
for bit on inputs made here and on the simulator's own exports."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, I = np.float32, np.int32
GAMMA = 0.998
STATS, SIDE = 14, 5
OUT, TRACKED, WAITING = 0, 1, 2
ROW_KEYS = ("ret", "disc", "gpow", "len", "type", "phase")
WORLD_KEYS = ("world_hider_team", "world_phase")


def new_state(worlds, A, phase=OUT):
    rows = worlds * A
    return dict(ret=np.zeros(rows, F), disc=np.zeros(rows, F), gpow=np.ones(rows, F), len=np.zeros(rows, I), type=np.zeros(rows, I),
                phase=np.full(rows, phase, I), world_hider_team=np.zeros(worlds, I), world_phase=np.zeros(worlds, I))


def episode_step(st, table, A, reward, done, self_type, mask, result, hider_team, gamma, booked=None):
    """The contract: every row operation an explicit IEEE f32 operation in the stated order, selects where it says select;
    `st` (new_state) is updated in place, `table` [14] f64 is added to.  `booked`, if given, is a pair of lists (seekers,
    hiders) that receive the f32 discounted returns of the episodes that end, for the bound on their sum.  Returns
    (ended, restart), bool [rows]."""
    reward, mask = np.asarray(reward, F), np.asarray(mask, F)
    done, self_type, hider_team = np.asarray(done), np.asarray(self_type), np.asarray(hider_team)
    g = F(gamma)
    phase = st["phase"].copy()
    was = phase == TRACKED
    with np.errstate(all="ignore"):
        R = np.where(was, reward, F(0))
        ret = np.where(was, st["ret"] + R, st["ret"])
        disc = np.where(was, st["disc"] + st["gpow"] * R, st["disc"])
        gpow = np.where(was, st["gpow"] * g, st["gpow"])
    assert ret.dtype == F and disc.dtype == F and gpow.dtype == F
    length = np.where(was, st["len"] + 1, st["len"]).astype(I)
    ended = was & (done != 0)
    for side in (0, 1):
        sel = ended & ((st["type"] != 0) == bool(side))
        r = ret[sel].astype(np.float64)
        o = side * SIDE
        table[o] += sel.sum()
        table[o + 1] += r.sum()
        table[o + 2] += (r * r).sum()
        table[o + 3] += disc[sel].astype(np.float64).sum()
        table[o + 4] += length[sel].astype(np.float64).sum()
        if booked is not None:
            booked[side].extend(disc[sel].tolist())
    restart = (done != 0) | ((phase != WAITING) & (~was | (mask == 0)))
    st["ret"] = np.where(restart, F(0), ret)
    st["disc"] = np.where(restart, F(0), disc)
    st["gpow"] = np.where(restart, F(1), gpow)
    st["len"] = np.where(restart, 0, length).astype(I)
    st["type"] = np.where(restart, self_type, st["type"]).astype(I)
    st["phase"] = np.where(restart, np.where(mask != 0, TRACKED, OUT), phase).astype(I)
    worlds = ended.size // A
    w_end, w_restart = ended.reshape(worlds, A).any(1), restart.reshape(worlds, A).any(1)
    h = st["world_hider_team"]
    known = w_end & (st["world_phase"] == 1) & ((h == 0) | (h == 1))
    x = np.asarray(result, F).reshape(worlds, 2)[np.arange(worlds), np.clip(h, 0, 1)]
    table[10] += (known & (x == 1.0)).sum()
    table[11] += (known & (x == 0.0)).sum()
    table[12] += (known & (x == 0.5)).sum()
    table[13] += w_end.sum()
    latch = w_end | w_restart
    st["world_hider_team"] = np.where(latch, hider_team, h).astype(I)
    st["world_phase"] = np.where(latch, 1, st["world_phase"]).astype(I)
    return ended, restart


def synthetic_calls(worlds, A, calls, seed=0):
    """A run to test on, a list of per-call input dicts: rewards from {-11, -1, 0, 1}; worlds whose episodes last 5 + w % 7
    steps, staggered; with every episode a world draws how many of its rows are active and whether its teams are
    flipped.  As the simulator does it: done is written for the rows active in the episode that ends (the others keep
    what they had), self_type / self_mask / hider_team exported with a done are the next episode's, episode_result is
    that of the episode that ended, a row that is out carries a NaN reward.  The first call's done is stale noise."""
    rng = np.random.default_rng([seed, worlds, A, calls])
    rows = worlds * A
    period = 5 + np.arange(worlds) % 7
    age = rng.integers(0, period)                             # steps the running episode has had
    slot = np.tile(np.arange(A), worlds)

    def draw():
        return rng.integers(1, A + 1, worlds), rng.integers(0, 2, worlds)
    active, flip = draw()
    done = (rng.random(rows) < 0.3).astype(I)
    result = np.zeros((worlds, 2), F)
    out = []
    for _ in range(calls):
        age = age + 1
        over = age >= period
        mask_old = (slot < np.repeat(active, A))
        reward = rng.choice(np.array([-11, -1, 0, 1], F), rows).astype(F)
        reward[~mask_old] = np.nan
        done = np.where(mask_old, np.repeat(over, A).astype(I) * rng.choice(np.array([1, 7], I), rows), done).astype(I)
        outcome = rng.choice(np.array([0.0, 0.5, 1.0], F), worlds)
        result = np.where(over[:, None], np.stack([outcome, F(1) - outcome], 1), np.where((age == 1)[:, None], F(0), result)).astype(F)
        na, nf = draw()
        active, flip = np.where(over, na, active), np.where(over, nf, flip)
        age = np.where(over, 0, age)
        mask = (slot < np.repeat(active, A)).astype(F)
        # seekers first where flipped: the hiders are team 1 there; the first half of a world's rows is the first team
        first = slot < (A + 1) // 2
        self_type = np.where(np.repeat(flip, A) == 1, ~first, first).astype(I)
        out.append(dict(reward=reward, done=done.copy(), self_type=self_type, self_mask=mask, episode_result=result.copy(), hider_team=flip.astype(I)))
    return out


def run(calls, worlds, A, gamma=GAMMA, phase=OUT, booked=None):
    st, table = new_state(worlds, A, phase), np.zeros(STATS)
    for c in calls:
        episode_step(st, table, A, c["reward"], c["done"], c["self_type"], c["self_mask"], c["episode_result"], c["hider_team"], gamma, booked)
    return st, table


def _one_row(rewards, dones, masks=None, types=None, gamma=GAMMA, phase=OUT, first=None):
    """One world of one row through the calls; returns (state, table).  `first` is an arming call (mask 1, no done)."""
    n = len(rewards)
    masks = [1.0] * n if masks is None else masks
    types = [1] * n if types is None else types
    st, table = new_state(1, 1, phase), np.zeros(STATS)
    if first is not None:
        episode_step(st, table, 1, [np.nan], [0], [first], [1.0], np.zeros((1, 2), F), [0], gamma)
    for r, d, m, t in zip(rewards, dones, masks, types):
        episode_step(st, table, 1, [r], [d], [t], [m], np.zeros((1, 2), F), [0], gamma)
    return st, table


# ---- properties of the restatement ----
def test_constant_reward_one_gives_return_equal_to_length():
    st, table = _one_row([1.0] * 37, [0] * 36 + [1], first=1)
    assert table[SIDE + 0] == 1 and table[SIDE + 1] == 37 and table[SIDE + 4] == 37 and table[SIDE + 2] == 37 * 37
    st, _ = _one_row([1.0] * 20, [0] * 20, first=1)
    assert st["ret"][0] == 20 and st["len"][0] == 20


def test_gamma_one_gives_discounted_equal_to_plain_and_gamma_zero_the_first_reward():
    rng = np.random.default_rng(5)
    r = rng.standard_normal(50).astype(F)
    st, table = _one_row(r, [0] * 49 + [1], gamma=1.0, first=0)
    assert table[0] == 1 and table[3] == table[1] and table[1] != 0
    st, table = _one_row(r, [0] * 49 + [1], gamma=0.0, first=0)
    assert table[3] == float(r[0]) and table[1] != table[3]
    # and the discounted return against float64, within the roundings of 50 steps
    st, table = _one_row(r, [0] * 49 + [1], gamma=GAMMA, first=0)
    want = sum(float(F(GAMMA)) ** k * float(x) for k, x in enumerate(r))
    assert abs(table[3] - want) <= 3 * 50 * 2.0 ** -24 * np.abs(r).sum()


def test_an_out_row_with_stale_done_and_nan_reward_adds_nothing():
    st, table = _one_row([np.nan] * 6, [1] * 6, masks=[0.0] * 6)
    assert not table.any() and st["phase"][0] == OUT and st["ret"][0] == 0 and st["disc"][0] == 0 and st["len"][0] == 0
    assert np.isfinite(st["ret"]).all() and np.isfinite(st["disc"]).all()


def test_a_joining_row_with_done_zero_starts_at_zero():
    # out for three calls (NaN rewards), joins with done = 0 and a reward that belongs to nobody, then plays four steps
    st, table = _one_row([np.nan, np.nan, 5.0, 1.0, 1.0, 1.0, 1.0], [1, 1, 0, 0, 0, 0, 1], masks=[0, 0, 1, 1, 1, 1, 1])
    assert table[SIDE] == 1 and table[SIDE + 1] == 4 and table[SIDE + 4] == 4


def test_a_waiting_row_ignores_everything_until_its_first_done():
    st, table = _one_row([3.0] * 5 + [1.0] * 4, [0, 0, 0, 0, 1, 0, 0, 0, 1], masks=[1, 0, 1, 1, 1, 1, 1, 1, 1], phase=WAITING)
    assert table[SIDE] == 1 and table[SIDE + 1] == 4 and table[SIDE + 4] == 4 and table[13] == 1
    st, table = _one_row([3.0] * 5, [0] * 5, masks=[1, 0, 1, 0, 1], phase=WAITING)
    assert not table.any() and st["phase"][0] == WAITING and st["ret"][0] == 0


def test_flipped_teams_book_under_the_latched_type_and_team():
    # one world, two rows; episode 1: row 0 hider, hiders are team 0; the done step exports episode 2's flipped types and team
    st, table = new_state(1, 2), np.zeros(STATS)
    res0 = np.zeros((1, 2), F)
    episode_step(st, table, 2, [np.nan, np.nan], [0, 0], [1, 0], [1, 1], res0, [0], GAMMA)                  # arm
    episode_step(st, table, 2, [1.0, -1.0], [0, 0], [1, 0], [1, 1], res0, [0], GAMMA)
    episode_step(st, table, 2, [1.0, -1.0], [1, 1], [0, 1], [1, 1], np.array([[1.0, 0.0]], F), [1], GAMMA)   # team 0 won: the hiders
    assert table[SIDE] == 1 and table[SIDE + 1] == 2 and table[0] == 1 and table[1] == -2
    assert table[10] == 1 and table[11] == 0 and table[12] == 0 and table[13] == 1
    assert st["type"].tolist() == [0, 1] and st["world_hider_team"][0] == 1
    # episode 2: team 0 wins again, now the seekers
    episode_step(st, table, 2, [-1.0, 1.0], [1, 1], [0, 1], [1, 1], np.array([[1.0, 0.0]], F), [1], GAMMA)
    assert table[10] == 1 and table[11] == 1 and table[13] == 2 and table[1] == -3 and table[SIDE + 1] == 3


def test_synthetic_run_covers_what_it_is_for():
    calls = synthetic_calls(13, 5, 300)
    booked = ([], [])
    st, table = run(calls, 13, 5, booked=booked)
    assert table[0] > 50 and table[SIDE] > 50 and table[13] > 100 and min(table[10:13]) > 10
    assert table[10] + table[11] + table[12] == table[13]
    assert len(booked[0]) == table[0] and len(booked[1]) == table[SIDE]
    stale = sum(int(((c["self_mask"] == 0) & (c["done"] != 0)).sum()) for c in calls)
    nan = sum(int(np.isnan(c["reward"]).sum()) for c in calls)
    assert stale > 100 and nan > 100 and np.isfinite(table).all()
    assert len({tuple(c["hider_team"]) for c in calls}) > 10


# ---- request() ----
class _Sim:
    num_worlds, agents_per_world, gpu_id = 6, 4, 0


def test_request_refuses_before_the_library_is_called():
    import torch
    from gpu_hideseek import episodes as E
    W, A = _Sim.num_worlds, _Sim.agents_per_world
    R = W * A

    def call(state=None, table=None, **kw):
        st = E.new_state(W, A, "cpu")
        st.update(state or {})
        return E.compute(_Sim(), st, torch.zeros(E.STATS, dtype=torch.float64) if table is None else table, **kw)

    buf = torch.zeros(64, dtype=torch.float64)
    bad = [
        (dict(reward=torch.zeros(R, dtype=torch.float64)), "reward.*dtype"), (dict(done=torch.zeros(R)), "done.*dtype"),
        (dict(self_type=torch.zeros(R, dtype=torch.int64)), "self_type.*dtype"), (dict(self_mask=torch.zeros(R, dtype=torch.int32)), "self_mask.*dtype"),
        (dict(reward=torch.zeros(R + 1)), "reward.*shape"), (dict(done=torch.zeros(A, W, dtype=torch.int32)), "done.*shape"),
        (dict(self_mask=torch.zeros(2 * R)[::2]), "self_mask.*not contiguous"), (dict(reward=[0.0] * R), "reward"),
        (dict(episode_result=torch.zeros(W, 3)), "episode_result.*shape"), (dict(episode_result=torch.zeros(W, 2, dtype=torch.float64)), "episode_result.*dtype"),
        (dict(hider_team=torch.zeros(W + 1, dtype=torch.int32)), "hider_team.*shape"), (dict(hider_team=torch.zeros(W)), "hider_team.*dtype"),
        (dict(state=dict(ret=torch.zeros(R - 1))), "ret.*shape"), (dict(state=dict(len=torch.zeros(R))), "len.*dtype"),
        (dict(state=dict(world_phase=torch.zeros(R, dtype=torch.int32))), "world_phase.*shape"), (dict(state=dict(extra=torch.zeros(R))), "state must be"),
        (dict(table=torch.zeros(13, dtype=torch.float64)), "table.*shape"), (dict(table=torch.zeros(14)), "table.*dtype"),
        (dict(gamma=float("nan")), "gamma"), (dict(gamma=float("inf")), "gamma"), (dict(gamma=1.5), "gamma"), (dict(gamma=-0.01), "gamma"),
        # a state tensor in the table's storage
        (dict(state=dict(ret=buf.view(torch.float32)[:R]), table=buf[:14]), "table overlaps ret"),
        (dict(state=dict(disc=buf.view(torch.float32)[4:4 + R], phase=buf.view(torch.int32)[R:2 * R])), "phase overlaps disc"),
        (dict(state=dict(gpow=buf.view(torch.float32)[:R]), reward=buf.view(torch.float32)[R - 1:2 * R - 1]), "gpow overlaps reward"),
    ]
    for kw, what in bad:
        with pytest.raises(ValueError, match=what):
            call(**kw)
    # well formed, on the wrong device: every accepted shape gets as far as the device check
    for shape in ((R,), (R, 1), (W, A)):
        with pytest.raises(ValueError, match="reward must be on cuda:0: it is on cpu"):
            call(reward=torch.zeros(shape), done=torch.zeros(shape, dtype=torch.int32), self_type=torch.zeros(shape, dtype=torch.int32),
                 self_mask=torch.zeros(shape), episode_result=torch.zeros(W, 2), hider_team=torch.zeros(W, dtype=torch.int32))
    with pytest.raises(ValueError, match="ret must be on cuda:0: it is on cpu"):
        call()
    with pytest.raises(ValueError, match="gamma"):
        E.EpisodeStats(_Sim(), gamma=2.0)


# ---- stats_to_metrics ----
def test_stats_to_metrics_against_float64_and_zero_for_empty_counts():
    import torch
    from gpu_hideseek import episodes as E
    rng = np.random.default_rng(9)
    rs, rh = rng.standard_normal(7) * 30, rng.standard_normal(11) * 30 + 4
    ds, dh, ls, lh = rs * 0.8, rh * 0.8, rng.integers(1, 241, 7), rng.integers(1, 241, 11)
    t = np.array([7, rs.sum(), (rs * rs).sum(), ds.sum(), ls.sum(), 11, rh.sum(), (rh * rh).sum(), dh.sum(), lh.sum(), 5, 2, 1, 8], np.float64)
    for table in (torch.from_numpy(t), t.tolist()):
        m = E.stats_to_metrics(table)
        for name, r, d, l in (("seekers", rs, ds, ls), ("hiders", rh, dh, lh)):
            s = m[name]
            assert s["episodes"] == len(r) and abs(s["return_mean"] - r.mean()) < 1e-12 and abs(s["return_std"] - r.std()) < 1e-10
            assert abs(s["discounted_return_mean"] - d.mean()) < 1e-12 and abs(s["length_mean"] - l.mean()) < 1e-12
        assert m["world_episodes"] == 8 and m["hider_win_rate"] == 5 / 8 and m["seeker_win_rate"] == 2 / 8 and m["draw_rate"] == 1 / 8
    none = E.stats_to_metrics(torch.zeros(14, dtype=torch.float64))
    flat = [v for side in ("seekers", "hiders") for v in none[side].values()] + [none[k] for k in ("world_episodes", "hider_win_rate", "seeker_win_rate", "draw_rate")]
    assert len(flat) == 14 and all(v == 0.0 and not math.isnan(v) for v in flat)
    half = E.stats_to_metrics([0, 0, 0, 0, 0, 2, 6.0, 18.0, 4.0, 480, 0, 0, 0, 0])      # hiders only, and no world finished
    assert half["seekers"]["return_mean"] == 0.0 and half["hiders"]["return_mean"] == 3.0 and half["hiders"]["return_std"] == 0.0
    assert half["hiders"]["length_mean"] == 240 and half["hider_win_rate"] == 0.0
    with pytest.raises(ValueError, match="table"):
        E.stats_to_metrics(torch.zeros(13))


# ---- the header ----
def test_header_mirror_and_symbols_agree(hideseek_lib):
    from gpu_hideseek import episodes as E
    src = open(os.path.join(ROOT, "include", "hideseek.h")).read()
    flat = " ".join(src.split())
    assert "int32_t hs_episode_stats(hs_sim *sim, const hs_episode_request *req);" in flat
    assert "int32_t hs_episode_stats_async(hs_sim *sim, void *hip_stream, const hs_episode_request *req);" in flat
    enums = dict(re.findall(r"(HS_EPISODE_[A-Z_]+) = (\d+)", src))
    assert enums == {"HS_EPISODE_STATS": "14", "HS_EPISODE_SIDE_STATS": "5", "HS_EPISODE_OUT": "0", "HS_EPISODE_TRACKED": "1", "HS_EPISODE_WAITING": "2"}
    assert (E.STATS, E.SIDE_STATS, E.OUT, E.TRACKED, E.WAITING) == (14, 5, 0, 1, 2)
    assert (E.STATS, E.SIDE_STATS, E.OUT, E.TRACKED, E.WAITING) == (STATS, SIDE, OUT, TRACKED, WAITING)
    assert (E.HIDER_WINS, E.SEEKER_WINS, E.DRAWS, E.WORLD_EPISODES) == (10, 11, 12, 13) and (E.SEEKER, E.HIDER) == (0, 1)
    body = re.search(r"typedef struct hs_episode_request \{(.*?)\} hs_episode_request;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in E.HsEpisodeRequest._fields_]
    want = dict(reward=0, done=8, self_type=16, self_mask=24, episode_result=32, hider_team=40, gamma=48, reserved=52, ret=56, disc=64, gpow=72,
                len=80, type=88, phase=96, world_hider_team=104, world_phase=112, table=120)
    assert C.sizeof(E.HsEpisodeRequest) == 128
    assert {n: getattr(E.HsEpisodeRequest, n).offset for n in want} == want
    assert [k for k, _ in E.ROW_STATE + E.WORLD_STATE] == names[8:16] == list(ROW_KEYS + WORLD_KEYS)
    L = C.CDLL(hideseek_lib)
    assert hasattr(L, "hs_episode_stats") and hasattr(L, "hs_episode_stats_async")
