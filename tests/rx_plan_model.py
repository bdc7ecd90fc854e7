"""The receive launch's dispatch rules and geometry a second time, in Python, for
tests/test_rx_plan_model.py to compare hackrfdiags_amd/csrc/hrfd_rx_plan.h against, step by step.

Written from the design's statement of the rules, kind by kind, not from the header's control flow:

* A call is a BATCH when it has more than one block and is neither the exact replay (serial), the inner API (src256) nor
  a subset.  A batch has the FLOW SHAPE when the flow kernel is allowed (use_stream 2), its tables are proven (first-octant
  and first-quadrant), the table gather is not forced (atan_mode 0) and a block is whole units of 512 samples at 256 kS/s,
  at least four of them.
* WBFM channels of a call with the flow shape always run on the flow kernel.  AM/SSB and FM channels do when the call has
  at most 64 blocks and the hook allows it (fir_flow: 0 never, -1 from 48 channels of the kind, 1 and 2 always).
* Two kinds or more go as ONE bank launch (list 9) instead, under the same conditions, from 48 channels with a demodulator
  (fir_flow 1: always; fir_flow 2: never).
* A kind that does not run on a flow kernel runs on the block kernels, and k_rx_finish finishes it; mode NONE always does.
* Behind every flow launch of at most 64 blocks comes the gated pass of its kinds when a squelch gate can close at all:
  the highest threshold above -42 - gain_db dBFS.
"""
from collections import namedtuple

NONE, AM, FM, WBFM, LSB, USB = range(6)
LIST_SUBSET, LIST_AS, LIST_BANK = 6, 7, 9
THREADS, TILE, NEED_HIST, MAX_TILES, MAX_HAL, DBG_SLOTS = 1024, 70, 644, 256, 1280, 48
WARM_TILES, SEED_TERMS, WARM_DEFAULT, FLOW_WARM_TILES = 3, 5, 512, 2
EINVAL, ESTATE = -1, -4

Step = namedtuple("Step", "kernel list n_list grid block run_len n_runs warm_tiles self_finish dbg expire_once")
FIELDS = ("n_none n_am n_fm n_wb n_lsb n_usb n_blocks n256 gain_db max_threshold warm_tiles serial src256 subset dump "
          "use_stream atan_mode fir_flow gated_pass run_len tab_ok quad_ok arith_ok has_dbg dbg_cap").split()
Case = namedtuple("Case", FIELDS)


def ceil_div(a, b):
    return -(-a // b)


def groups(n):
    return 8 * ceil_div(n, 8)


def longest_run(n_blocks, n, forced, longest, fill):
    """Blocks per workgroup: the forced length, or the longest up to `longest` that still gives `fill` workgroups."""
    if forced > 0:
        return min(forced, n_blocks)
    for run in range(min(longest, n_blocks), 1, -1):
        if groups(n) * ceil_div(n_blocks, run) >= fill:
            return run
    return 1


def plan(c):
    count = {NONE: c.n_none, AM: c.n_am, FM: c.n_fm, WBFM: c.n_wb, LSB: c.n_lsb, USB: c.n_usb}
    n_as = c.n_am + c.n_lsb + c.n_usb
    kind_count = {"as": n_as, "fm": c.n_fm, "wb": c.n_wb}
    kind_list = {"as": LIST_AS, "fm": FM, "wb": WBFM}
    total = sum(count.values())
    batch = c.n_blocks > 1 and not (c.serial or c.src256 or c.subset)
    shape = (batch and c.use_stream == 2 and c.tab_ok and c.quad_ok and c.atan_mode != 0 and c.n256 % 512 == 0
             and c.n256 >= 2048)
    fir_ok = shape and c.n_blocks <= 64 and c.fir_flow != 0
    present = [k for k in ("as", "fm", "wb") if kind_count[k]]
    bank = fir_ok and len(present) >= 2 and (c.fir_flow == 1 or (c.fir_flow == -1 and total - c.n_none >= 48))
    on_flow = {"wb": shape, "as": fir_ok and (c.fir_flow > 0 or n_as >= 48), "fm": fir_ok and (c.fir_flow > 0 or c.n_fm >= 48)}
    gate_can_close = c.gated_pass and c.n_blocks <= 64 and c.max_threshold > -42 - c.gain_db
    flow_warm = min(c.warm_tiles, FLOW_WARM_TILES)
    dump = "_dump" if c.dump else ""
    theta = "_256" if c.src256 else "_arith" if (c.arith_ok and c.atan_mode != 0) else ""
    steps = []
    flows = [0]

    def with_dbg(grid):
        return bool(c.has_dbg and grid * DBG_SLOTS <= c.dbg_cap)

    def flow(kernel, lst, n, run):
        n_runs = ceil_div(c.n_blocks, run)
        grid = groups(n) * n_runs
        steps.append(Step(kernel + dump, lst, n, grid, THREADS, run, n_runs, flow_warm, True, with_dbg(grid), flows[0] == 0))
        flows[0] += 1

    def gated(kinds):
        for k in kinds:
            if gate_can_close and kind_count[k]:
                steps.append(Step("gated_" + k, kind_list[k], kind_count[k], groups(kind_count[k]), THREADS, c.n_blocks, 1,
                                  flow_warm, True, False, False))

    def block_kernel(kernel, lst, n, wants_dbg):
        run = 1 if (c.serial or c.src256) else longest_run(c.n_blocks, n, c.run_len, 8, 512)
        n_runs = ceil_div(c.n_blocks, run)
        grid = groups(n) * n_runs
        steps.append(Step(kernel, lst, n, grid, THREADS, run, n_runs, c.warm_tiles, False, wants_dbg and with_dbg(grid), False))

    def per_block(kernel, lst, n):
        steps.append(Step(kernel, lst, n, groups(n) * c.n_blocks, THREADS, 1, c.n_blocks, c.warm_tiles, False, False, False))

    if bank:
        flow("flow_bank", LIST_BANK, total - c.n_none, c.n_blocks)
        gated(["wb", "fm", "as"])
        finished_inside = {AM, FM, WBFM, LSB, USB}
    else:
        finished_inside = set()
        for k in ("as", "fm", "wb"):
            n = kind_count[k]
            if not n:
                continue
            if on_flow[k]:
                run = longest_run(c.n_blocks, n, c.run_len, 64, 256) if k == "wb" else c.n_blocks
                flow("flow_" + k, kind_list[k], n, run)
                gated([k])
                finished_inside |= {"as": {AM, LSB, USB}, "fm": {FM}, "wb": {WBFM}}[k]
            elif k == "as":
                per_block("fir_as" + ("_256" if c.src256 else ""), LIST_AS, n)
                steps.append(Step("post_as", LIST_AS, n, n, 256, 1, c.n_blocks, c.warm_tiles, False, False, False))
            elif k == "fm":
                per_block("fir_fm" + theta, FM, n)
            else:
                block_kernel("blocks_wb" + theta, WBFM, n, True)
    if c.n_none:
        block_kernel("blocks_none", NONE, c.n_none, False)

    def finish(lst, n):
        if n:
            steps.append(Step("finish", lst, n, n, 64, 1, c.n_blocks, c.warm_tiles, False, False, False))

    if c.subset:
        finish(LIST_SUBSET, total)
    elif not finished_inside:
        finish(-1, total)
    else:
        for m in (NONE, AM, FM, WBFM, LSB, USB):
            if m not in finished_inside:
                finish(m, count[m])
    return steps


def finished_by(step, case):
    """The modes whose channels a finishing step finishes."""
    return {LIST_BANK: (AM, FM, WBFM, LSB, USB), LIST_AS: (AM, LSB, USB), LIST_SUBSET: tuple(range(6)), -1: tuple(range(6))}.get(
        step.list, (step.list,))


# ---------------------------------------------------------------- geometry
def geometry(block_bytes, n_blocks, stride, out_b0, out_blocks, serial, src256, offgrid, warm):
    """(code, text) of a refusal, or (0, (ragged, n256, warm_tiles, seed_terms, ntiles, origin, hal))."""
    top = 32768 if src256 else 262144
    if block_bytes == 0 or block_bytes % 2 or block_bytes > top:
        return EINVAL, "%s must be even, > 0 and <= %d (got %d)" % ("bytes_per_channel" if src256 else "block_bytes", top, block_bytes)
    if n_blocks == 0 or out_b0 + n_blocks > out_blocks:
        return EINVAL, "bad block count"
    if stride < block_bytes * n_blocks:
        return EINVAL, "channel_stride smaller than n_blocks*block_bytes"
    if block_bytes * n_blocks > 2 ** 31 - 1:
        return EINVAL, "n_blocks*block_bytes = %d exceeds 2^31 - 1 bytes per channel and call" % (block_bytes * n_blocks)
    per_sample = 2 if src256 else 16
    ragged = bool(offgrid) or block_bytes % (64 * per_sample) != 0
    n256 = block_bytes // per_sample
    warm_tiles, seed_terms = (WARM_TILES, SEED_TERMS) if warm >= WARM_DEFAULT else (min(WARM_TILES, warm // 128), 0)
    # tiles of 70 samples that end at n256; tile number warm_tiles + seed_terms starts at or before sample -(644 + 1)
    ntiles = ceil_div(n256 + NEED_HIST + 1, TILE) + warm_tiles + seed_terms
    origin = n256 - TILE * ntiles
    hal = 64 * ceil_div(-origin, 64)
    if not ragged:
        if ntiles > MAX_TILES:
            return EINVAL, "internal: %d de-emphasis tiles exceed %d" % (ntiles, MAX_TILES)
        if hal > MAX_HAL:
            return EINVAL, "internal: history %d exceeds %d" % (hal, MAX_HAL)
        if n_blocks > 1 and (hal + 64) * per_sample > block_bytes:
            return EINVAL, ("blocks of %d bytes are too short for a multi-block call (need >= %d); submit them one per call"
                            % (block_bytes, (hal + 64) * per_sample))
    if serial and n_blocks != 1:
        return ESTATE, "internal: serial replay needs n_blocks == 1"
    return 0, (int(ragged), n256, warm_tiles, seed_terms, ntiles, origin, hal)
