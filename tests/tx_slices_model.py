"""The modulator launch's refusal, time slices and grids a second time, in Python, for
tests/test_tx_slices_model.py to compare hackrfdiags_amd/csrc/hrfd_tx_slices.h against.  Python's integers do not wrap: a
grid of the header that equals the model's was computed without a wrap.

* Lengths of slices are in UNITS of 64 input samples; the cascade's tile is 128 samples, so every cut but the call's end
  is an even number of units.
* WBFM: a call of more than 24 units (counted even, rounded down) is cut: 2 and 8 units at the head, 4 and 2 at the tail
  (16, 8, 4, 2 from 72 units), and between them the rest in even shares of at least 32 units, as few as fit the handle's 32
  event pairs.  The last slice ends with the call.
* FM: a call of 64 units or more is cut into three slices: a sixteenth of the call (at least 8 units, even, rounded up),
  three and a half times that (what is left less two units if that is shorter, even, rounded down), the rest.
* A call is accepted when its cascade fits one launch -- 8 ceil(C / 8) ceil(n / 128) workgroups of 256 threads, at most
  (2^32 - 1) / 256 of them -- and, WBFM only, when 32 n cells plus a tile of 32 * 128 stay within a signed 32-bit index.
"""
import itertools

SSB, INTERP, AM, FM, WBFM, SIG_AM, SIG_DSB, SIG_PM, SIG_FM = range(1, 10)
EINVAL = -1
TILE, UNIT, MAX_SLICES = 128, 64, 32
MAX_WGS = (2 ** 32 - 1) // 256
WBFM_MAX_N = (2 ** 31 - 1) // 32 - TILE


def ceil_div(a, b):
    return -(-a // b)


def even_up(x):
    return x + (x & 1)


def wbfm_units(n):
    return ceil_div(n, UNIT) & ~1


def wbfm_sliceable(n):
    return wbfm_units(n) > 24


def wbfm_cuts(n, max_slices=MAX_SLICES):
    nt = wbfm_units(n)
    if nt <= 24:
        return [n]
    head, tail = [2, 8], ([16, 8, 4, 2] if nt >= 72 else [4, 2])
    mid = nt - sum(head) - sum(tail)
    room = max_slices - len(head) - len(tail) - 1
    piece = max(32, ceil_div(mid, room))
    lens = list(head)
    while mid:
        share = min(mid, even_up(ceil_div(mid, ceil_div(mid, piece))))
        lens.append(share)
        mid -= share
    ends = list(itertools.accumulate(lens + tail))
    return [UNIT * e for e in ends[:-1]] + [n]


def fm_sliceable(n):
    return ceil_div(n, UNIT) >= 64


def fm_cuts(n):
    nt = ceil_div(n, UNIT)
    l0 = even_up(max(8, nt // 16))
    l1 = min(7 * l0 // 2, nt - l0 - 2) & ~1
    return [0, UNIT * l0, UNIT * (l0 + l1), n]


def mod_grid(C, length):
    return 8 * ceil_div(C, 8) * ceil_div(length, TILE)


def base_grid(C, length):
    return ceil_div(C * length, 256)


def wb_tail_grid(C, span, max_wgs):
    items = ceil_div(C, 8) * ceil_div(32 * span, 2048)     # a wave per item of 2048 cells, on the fullest of the 8 XCDs
    return 8 * max(1, min(max_wgs // 8, ceil_div(items, 1024 // 64)))


def wb_rails_grid(C, span, max_wgs):
    return min(max_wgs, ceil_div(8 * span * C, 512))          # four cells per thread, 512 threads


def scan(scan_kind, C, steps, stride, rows8=True):
    """(kernel, grid) of the phase recurrence"""
    if scan_kind != 1 and C <= 8192 and steps % 64 == 0 and stride < 2 ** 28:
        return ("rows8" if scan_kind != 2 and rows8 and steps % 128 == 0 else "rows"), ceil_div(C, 16)
    return ("scan64" if steps % 4 == 0 and stride % 4 == 0 else "plain"), ceil_div(C, 64)


def accepted(kind, C, n):
    return mod_grid(C, n) <= MAX_WGS and (kind != WBFM or n <= WBFM_MAX_N)


def max_n(kind, C):
    """the longest call of C channels that is accepted (0: none)"""
    n = TILE * (MAX_WGS // (8 * ceil_div(C, 8)))
    return min(n, WBFM_MAX_N) if kind == WBFM else n


def grids(kind, C, n, scan_kind=0):
    """the harness's line for an accepted call, as a list of tokens"""
    out = ["0", "mod", mod_grid(C, n), "base", base_grid(C, n)]
    if kind == WBFM:
        out += ["tail", wb_tail_grid(C, n, 512), "rails", wb_rails_grid(C, n, 512), *scan(scan_kind, C, 32 * n, 32 * n)]
        cuts = wbfm_cuts(n)
        for lo, hi in zip([0] + cuts, cuts) if len(cuts) > 1 else ():
            out += ["|", mod_grid(C, hi - lo), wb_tail_grid(C, hi - lo, 384), wb_rails_grid(C, hi - lo, 384),
                    *scan(scan_kind, C, 32 * (hi - lo), 32 * n)]
    if kind == FM:
        out += [*scan(scan_kind, C, n, n)]
        cuts = fm_cuts(n) if fm_sliceable(n) else []
        for lo, hi in zip(cuts, cuts[1:]):
            out += ["|", mod_grid(C, hi - lo), base_grid(C, hi - lo), *scan(scan_kind, C, hi - lo, n)]
    return [str(x) for x in out]
