"""The two dispatch computations tests/test_gpu_bank_launch_shapes.py rests on, restated as plain functions and checked for
every shape that file names: the tone generator's grid (tonegen_launch and k_tonegen's tile loop in
hackrfdiags_amd/csrc/hrfd_tonegen.hip), its staging uploads (tonegen_stage), and the conditioner's share per workgroup and
steps per lane (cal_launch, k_cal and cal_groups in hackrfdiags_amd/csrc/hrfd_cal.hip).  No device: this pins that the shapes
reach the paths they are chosen for -- a second tile in one workgroup, a second upload, the widening inside the loop.  The
GPU file imports these functions and asserts the same figures next to the calls it makes, so that a constant that moves in
the library fails an assertion there instead of leaving a test that no longer reaches its path."""
import pytest

TONEGEN_TILE_BLOCKS = 4                    # kTonegenTile / 512
TONEGEN_TILE = 2048
TONEGEN_MAX_GRID_Y = 64
TONEGEN_AIM_WGS = 2048
TONEGEN_STAGE_CHANNELS = 1024
CAL_THREADS = 256
CAL_DEPTH = 4
CAL_WIDEN = 2048
CAL_TARGET_WGS = 2048                      # hrfd_cal::target_wgs as shipped
CAL_STEP_MOST = 1 << 19                    # a step of 4 groups of 8 samples adds at most 32 x 128 x 128 to a partial

MIB = 1 << 20
CAL_PAST_WIDENING_BYTES = 132 * MIB + 10   # section C of the GPU file
CAL_PAST_WIDENING_RESIDUE = 6

# (C, n_blocks, gy): the shapes of the GPU file's tile tests
TONEGEN_SHAPES = [(1, 257, 64), (3, 515, 64), (1, 1024, 64), (700, 13, 3), (1024, 9, 2), (1024, 16, 2), (2049, 5, 1)]


def ceil_div(a, b):
    return -(-a // b)


def tonegen_dispatch(C, n_blocks):
    """(tiles, want, gy) of tonegen_launch"""
    tiles = ceil_div(n_blocks, TONEGEN_TILE_BLOCKS)
    want = ceil_div(TONEGEN_AIM_WGS, C)
    return tiles, want, min(tiles, TONEGEN_MAX_GRID_Y, max(want, 1))


def tonegen_tiles_of(C, n_blocks, y):
    """the tiles workgroup (c, y) walks: t0 = y * 2048, then += gridDim.y * 2048 while below n"""
    tiles, _, gy = tonegen_dispatch(C, n_blocks)
    return list(range(y, tiles, gy))


def tonegen_tile_blocks(n_blocks, tile):
    """the blocks of a tile: 4 but for the last one"""
    return min(TONEGEN_TILE_BLOCKS, n_blocks - TONEGEN_TILE_BLOCKS * tile)


def tonegen_uploads(lo, hi):
    """[(first channel, count)] of tonegen_stage over the dirty range lo .. hi - 1: counted from lo, not from 0"""
    return [(c0, min(hi - c0, TONEGEN_STAGE_CHANNELS)) for c0 in range(lo, hi, TONEGEN_STAGE_CHANNELS)]


def cal_dispatch(n_bytes, W, target_wgs=CAL_TARGET_WGS):
    """(groups_per_wg, wg_per_capture) of cal_launch"""
    groups = n_bytes // 16
    rounds = ceil_div(groups, CAL_THREADS)
    want = max(1, target_wgs // W)
    per = max(CAL_DEPTH, ceil_div(rounds, want))
    per = ceil_div(per, CAL_DEPTH) * CAL_DEPTH
    groups_per_wg = per * CAL_THREADS
    return groups_per_wg, max(1, ceil_div(groups, groups_per_wg))


def cal_row(n_bytes, residue):
    """(head bytes, whole groups, tail bytes) of a row at an address of the given residue modulo 16, as k_cal splits it"""
    head = min(n_bytes, (0 - residue) & 15) if residue % 2 == 0 else 0
    groups = (n_bytes - head) >> 4
    return head, groups, n_bytes - head - 16 * groups


def cal_steps(n_bytes, residue, W, target_wgs=CAL_TARGET_WGS):
    """the most steps of cal_groups' loop a lane of each of a capture's workgroups takes: a step is kCalDepth groups
    256 apart, lane tid starts at g0 + tid"""
    groups_per_wg, wgs = cal_dispatch(n_bytes, W, target_wgs)
    _, groups, _ = cal_row(n_bytes, residue)
    steps = []
    for j in range(wgs):
        g0, g1 = j * groups_per_wg, min(groups, (j + 1) * groups_per_wg)
        steps.append(ceil_div(max(g1 - g0, 0), CAL_THREADS * CAL_DEPTH))
    return steps


# ------------------------------------------------------------------ the tone generator's tiles
@pytest.mark.parametrize("C,n_blocks,gy", TONEGEN_SHAPES)
def test_tonegen_shapes_put_several_tiles_into_one_workgroup(C, n_blocks, gy):
    tiles, want, got = tonegen_dispatch(C, n_blocks)
    assert got == gy and tiles > gy, (tiles, want, got)
    mine = tonegen_tiles_of(C, n_blocks, 0)
    assert len(mine) >= 2 and mine[1] == gy
    # every tile belongs to exactly one workgroup of the row
    taken = sorted(t for y in range(gy) for t in tonegen_tiles_of(C, n_blocks, y))
    assert taken == list(range(tiles))
    assert 1024 * n_blocks * C <= 16 * MIB


def test_tonegen_shapes_are_what_the_issue_says_of_them():
    assert tonegen_tiles_of(1, 257, 0) == [0, 64] and tonegen_tile_blocks(257, 64) == 1      # only wave 0 is live in tile 64
    assert tonegen_tiles_of(3, 515, 0) == [0, 64, 128] and tonegen_tile_blocks(515, 128) == 3
    assert all(len(tonegen_tiles_of(1, 1024, y)) == 4 for y in range(64))                    # the largest call
    assert tonegen_tiles_of(700, 13, 0) == [0, 3] and tonegen_tiles_of(700, 13, 1) == [1]
    assert tonegen_tiles_of(1024, 9, 0) == [0, 2] and tonegen_tiles_of(1024, 9, 1) == [1]
    assert tonegen_tiles_of(1024, 16, 0) == [0, 2] and tonegen_tiles_of(1024, 16, 1) == [1, 3]
    assert tonegen_tiles_of(2049, 5, 0) == [0, 1]                                            # one workgroup walks a whole row


def test_the_tone_generators_own_suite_never_had_a_second_tile():
    """what the issue says of tests/test_gpu_tonegen.py: its largest shapes have tiles <= gy"""
    for C, n_blocks in [(64, 16), (1, 32), (65, 9), (5, 5), (50, 24)]:
        tiles, _, gy = tonegen_dispatch(C, n_blocks)
        assert tiles == gy


# ------------------------------------------------------------------ the tone generator's uploads
def test_tonegen_staging_splits():
    assert tonegen_uploads(0, 2049) == [(0, 1024), (1024, 1024), (2048, 1)]                  # the create-time range
    assert tonegen_uploads(1023, 1026) == [(1023, 3)]                                        # one upload, not from 0
    assert tonegen_uploads(0, 65) == [(0, 65)]                                               # the most the bank's own suite has
    assert tonegen_uploads(1023, 2049) == [(1023, 1024), (2047, 2)]
    for lo, hi in ((0, 2049), (1023, 1026), (5, 4000)):
        covered = [c for c0, k in tonegen_uploads(lo, hi) for c in range(c0, c0 + k)]
        assert covered == list(range(lo, hi))


# ------------------------------------------------------------------ the conditioner's steps
def test_cal_one_workgroup_passes_the_widening_four_times():
    n, res = CAL_PAST_WIDENING_BYTES, CAL_PAST_WIDENING_RESIDUE
    assert cal_row(n, res) == (10, 132 * MIB // 16, 0)      # a head of 5 samples; the groups end with the row
    assert cal_dispatch(n, 1, 1) == (33792 * 256, 1)
    assert cal_steps(n, res, 1, 1) == [8448]
    assert divmod(8448, CAL_WIDEN) == (4, 256)               # four widenings in the loop and a remainder
    # the step count is derived: without the widening the signed partials wrap behind 4096 steps, the unsigned ones
    # behind 8192, and a widening that never resets `steps` is caught behind 2048 + 4096
    assert (1 << 31) // CAL_STEP_MOST == 4096 and (1 << 32) // CAL_STEP_MOST == 8192
    assert 8448 > 8192 and 8448 > CAL_WIDEN + 4096
    assert CAL_WIDEN * CAL_STEP_MOST == 1 << 30              # what kCalWiden keeps inside int32


def test_cal_three_workgroups_pass_it_once_each():
    n, res = CAL_PAST_WIDENING_BYTES, CAL_PAST_WIDENING_RESIDUE
    assert cal_dispatch(n, 1, 3) == (11264 * 256, 3)
    assert cal_steps(n, res, 1, 3) == [2816, 2816, 2816]
    assert divmod(2816, CAL_WIDEN) == (1, 768)


def test_cal_own_suite_stays_below_the_widening():
    """what the issue says of tests/test_gpu_cal.py: 64 steps under debug_set_workgroups(1) over a MiB, and the shipped
    state reaches 2048 steps only above 32 MiB of one capture in one workgroup's share"""
    assert cal_steps(MIB + 10, 6, 1, 1) == [64]
    assert max(cal_steps(MIB + 10, 6, 1)) < CAL_WIDEN and max(cal_steps(1 << 30, 0, 1)) < CAL_WIDEN
    assert cal_steps(32 * MIB, 0, 1, 1) == [2048] and cal_steps(32 * MIB - 16, 0, 1, 1) == [2048]
