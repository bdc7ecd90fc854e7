"""The receive launch's plan, lists and geometry (hackrfdiags_amd/csrc/hrfd_rx_plan.h) on the CPU: the header compiled
into tests/cpp/san_rx_plan.cc under -fsanitize=address,undefined and compared with tests/rx_plan_model.py, step by step
and field by field, over full grids of small sets; two properties over every case that need no model; the lists against
brute force; the geometry against closed forms for every even block length."""
import itertools
import os
import shutil
import subprocess

import pytest

from tests import rx_plan_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
COUNTS = (0, 1, 7, 8, 9, 47, 48, 49)
N_BLOCKS = (1, 2, 63, 64, 65)
BLOCK_BYTES = (1024, 24576, 32768, 36864, 40960, 262144)   # n256 64, 1536, 2048, 2304 (no multiple of 512), 2560, 16384
DEFAULT = dict(n_none=0, n_am=0, n_fm=0, n_wb=0, n_lsb=0, n_usb=0, n_blocks=16, n256=16384, gain_db=0, max_threshold=-200,
               warm_tiles=3, serial=0, src256=0, subset=0, dump=0, use_stream=2, atan_mode=-1, fir_flow=-1, gated_pass=1,
               run_len=0, tab_ok=1, quad_ok=1, arith_ok=1, has_dbg=0, dbg_cap=0)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = str(tmp_path_factory.mktemp("rx_plan") / "san_rx_plan")
    base = ["g++", "-x", "c++", "-std=c++17", "-g", "-O1", "-o", out, os.path.join(HERE, "cpp", "san_rx_plan.cc")]
    b = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if b.returncode != 0 and ("cannot find" in b.stderr or "unrecognized" in b.stderr):
        b = subprocess.run(base, capture_output=True, text=True)   # no sanitizer runtime here: the comparison still runs
    assert b.returncode == 0, b.stderr[-2000:]
    return out


def run(exe, what, text):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, what], input=text, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    return r.stdout


def split_as(k, spread):
    """k AM / SSB channels as (AM, LSB, USB): all AM, or spread over the three modes"""
    return (k - 2 * (k // 3), k // 3, k // 3) if spread else (k, 0, 0)


def cases():
    def make(n_as=0, spread=0, block_bytes=None, **kw):
        d = dict(DEFAULT, **kw)
        d["n_am"], d["n_lsb"], d["n_usb"] = split_as(n_as, spread)
        if block_bytes is not None:
            d["n256"] = block_bytes // (2 if d["src256"] else 16)
        return M.Case(**d)

    P = itertools.product
    # 1. which kernel serves which kind: every count of every kind, block count, hook
    for a, f, w, none, nb, ff, us in P(COUNTS, COUNTS, COUNTS, (1,), (2, 64, 65), (-1, 0, 1, 2), (2,)):
        yield make(a, (a + f) % 2, n_fm=f, n_wb=w, n_none=none, n_blocks=nb, fir_flow=ff, use_stream=us)
    for a, f, w, none, nb, ff, us in P((0, 1, 9, 47, 48), (0, 7, 47, 48), (0, 8, 48, 49), (0, 1), N_BLOCKS, (-1, 0, 1, 2), (0, 2)):
        yield make(a, (a + f) % 2, n_fm=f, n_wb=w, n_none=none, n_blocks=nb, fir_flow=ff, use_stream=us)
    # 2. the block lengths, both entries
    for a, f, w, none, bb, nb, ff, us, s256 in P((0, 1, 48), (0, 1, 48), (0, 1, 48), (0, 9), BLOCK_BYTES, (1, 2, 65), (-1, 1),
                                                 (0, 2), (0, 1)):
        yield make(a, 1, n_fm=f, n_wb=w, n_none=none, block_bytes=bb, n_blocks=nb, fir_flow=ff, use_stream=us, src256=s256)
    # 3. the gated pass: the highest threshold at the detector's floor and one above it
    for a, f, w, gp, gain, above, nb, ff, dump in P((0, 8, 49), (0, 8, 49), (0, 8, 49), (0, 1), (0, 40), (0, 1), (2, 64, 65),
                                                    (-1, 1, 2), (0, 1)):
        yield make(a, 1, n_fm=f, n_wb=w, gated_pass=gp, gain_db=gain, max_threshold=-42 - gain + above, n_blocks=nb, fir_flow=ff,
                   dump=dump)
    # 4. the call's flags and the tables
    for flags, tabs, atan, (a, f, w), none, nb in P(P((0, 1), repeat=4), P((0, 1), repeat=3), (-1, 0, 1),
                                                    ((1, 1, 1), (48, 48, 48), (0, 0, 49), (7, 0, 9)), (0, 1), (1, 2, 16)):
        yield make(a, 1, n_fm=f, n_wb=w, n_none=none, n_blocks=nb, serial=flags[0], src256=flags[1], subset=flags[2], dump=flags[3],
                   tab_ok=tabs[0], quad_ok=tabs[1], arith_ok=tabs[2], atan_mode=atan, max_threshold=0)
    # 5. runs of blocks, the stamp buffer, a shrunk warm-up
    for rl, nb, w, a, none, us, (dbg, cap), warm in P((0, 1, 3, 64), N_BLOCKS, COUNTS, (0, 9), (0, 49), (0, 2),
                                                      ((0, 0), (1, 48 * 64), (1, 48 * 512)), (3,)):
        yield make(a, 0, n_wb=w, n_none=none, n_blocks=nb, run_len=rl, use_stream=us, has_dbg=dbg, dbg_cap=cap, warm_tiles=warm)
    for rl, nb, w, a, none, us, (dbg, cap), warm in P((0, 3), (2, 65), COUNTS, (9,), COUNTS, (0, 2), ((0, 0),), (3, 1)):
        yield make(a, 0, n_wb=w, n_none=none, n_blocks=nb, run_len=rl, use_stream=us, has_dbg=dbg, dbg_cap=cap, warm_tiles=warm)


def parse(out):
    plans = []
    for line in out.splitlines():
        t = line.split()
        if t[0] == "case":
            assert int(t[1]) == len(plans)
            plans.append([])
        else:
            v = [int(x) for x in t[1:]]
            plans[-1].append(M.Step(t[0], v[0], v[1], v[2], v[3], v[4], v[5], v[6], bool(v[7]), bool(v[8]), bool(v[9])))
    return plans


def test_plan_against_the_model(exe):
    """Every case of the grids: the header's steps equal the model's, and, without a model: every channel of every
    non-empty mode is finished exactly once -- inside the one flow launch that runs it, or by exactly one k_rx_finish (the
    gated launches redo channels of a flow launch and finish nobody else) -- and every grid is 8 ceil(n / 8) n_runs with
    n_runs run_len >= n_blocks (k_rx_post and k_rx_finish: a workgroup per channel)."""
    todo = list(cases())
    got = parse(run(exe, "plan", "".join(" ".join(str(int(x)) for x in c) + "\n" for c in todo)))
    assert len(got) == len(todo) > 30000
    for c, steps in zip(todo, got):
        want = M.plan(c)
        assert steps == want, (c, [s for s in zip(steps, want) if s[0] != s[1]][:1], len(steps), len(want))
        finished = [0] * 6
        for s in steps:
            if s.kernel in ("post_as", "finish"):
                assert s.grid == s.n_list
            else:
                assert s.grid == 8 * ((s.n_list + 7) // 8) * s.n_runs and s.n_runs * s.run_len >= c.n_blocks > (s.n_runs - 1) * s.run_len
            assert s.n_list > 0
            if s.kernel == "finish" or (s.self_finish and not s.kernel.startswith("gated")):
                for m in M.finished_by(s, c):
                    finished[m] += 1
        count = (c.n_none, c.n_am, c.n_fm, c.n_wb, c.n_lsb, c.n_usb)
        assert all(f == 1 for f, n in zip(finished, count) if n), (c, finished)


def test_lists_against_brute_force(exe):
    assert "san_rx_plan lists ok" in run(exe, "lists", "")


def test_geometry_against_closed_forms(exe):
    """ntiles, origin and hal for every even block length of both entries, and every refusal at its bound and to either
    side of it.  The two `internal:` refusals of the tiling (kMaxTiles, kMaxHal) cannot be reached by any length the first
    check lets through: the sweep shows that none appears."""
    calls = []
    for src256 in (0, 1):
        calls += [(bb, 1, bb, 0, 1, 0, src256, 0, 512) for bb in range(2, 262144 + 1, 2)]
        calls += [(bb, 2, 2 * bb, 0, 2, 0, src256, 0, 512) for bb in range(128, 262144 + 1, 128)]   # too short for two blocks?
        top = 32768 if src256 else 262144
        calls += [(bb, 1, bb, 0, 1, 0, src256, 0, 512) for bb in (0, 1, 3, top - 1, top + 1, top + 2)]
        for warm in (0, 2, 126, 128, 254, 256, 384, 510, 512):
            calls += [(bb, nb, nb * bb, 0, nb, 0, src256, 0, warm) for bb in (1024, 19456, 20480, 32768) for nb in (1, 2)]
        calls += [(4096, nb, 4096 * nb, b0, ob, 0, src256, 0, 512) for nb, b0, ob in
                  ((0, 0, 1), (1, 0, 0), (1, 0, 1), (1, 1, 1), (1, 1, 2), (3, 2, 4), (3, 2, 5), (3, 2, 6))]
        calls += [(4096, 3, 3 * 4096 + d, 0, 3, 0, src256, 0, 512) for d in (-1, 0, 1)]
        calls += [(2, nb, 2 ** 32, 0, nb, 0, src256, 1, 512) for nb in (2 ** 30 - 1, 2 ** 30)]
        calls += [(4096, nb, 4096 * nb, 0, nb, 1, src256, og, 512) for nb in (1, 2) for og in (0, 1)]
        calls += [(bb, 2, 2 * bb, 0, 2, 0, src256, 1, 512) for bb in (2, 1000, 1024, 32768)]
    out = run(exe, "geom", "".join(" ".join(map(str, c)) + "\n" for c in calls)).splitlines()
    assert len(out) == len(calls)
    refusals = set()
    for c, line in zip(calls, out):
        code, rest = line.split(" ", 1)
        want_code, want = M.geometry(*c)
        assert int(code) == want_code, (c, line, want)
        if want_code != 0:
            assert rest == want, (c, line, want)
            assert "tiles exceed" not in rest and "history" not in rest
            refusals.add(" ".join(rest.split(" ")[:2]))
        else:
            assert tuple(int(x) for x in rest.split()) == want, (c, line, want)
            ragged, n256, warm_tiles, seed_terms, ntiles, origin, hal = want
            # the tiling's own terms: the tiles end at n256, tile warm_tiles + seed_terms starts at or before -645, not a
            # whole tile before; the history covers tile 0 in whole waves
            first = origin + 70 * (warm_tiles + seed_terms)
            assert -645 - 70 < first <= -645 and origin + 70 * ntiles == n256 and 0 <= hal + origin < 64 and hal % 64 == 0
            assert ragged or (ntiles <= 256 and hal <= 1280)
    assert len(refusals) == 7, refusals                      # every other refusal of rx_geometry has been seen
