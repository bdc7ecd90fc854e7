// hackrfdiags_amd/csrc/hrfd_rx_plan.h -- what a receive launch decides before it touches the device: the geometry of
// the call, the per-mode channel lists, and the PLAN -- which kernel serves which list, with what grid, in what order
// (DESIGN.md 3.2a).  Pure functions: no HIP call, no handle, and no allocation (but in the experiment
// -DHRFD_BANK_XCD_ORDER=1, off by default).  Plain C++ (tests/cpp/san_rx_plan.cc compiles it on the CPU and
// tests/rx_plan_model.py states the same rules a second time); the includer declares
// `int fail(int code, const char *fmt, ...)` and the HRFD_* codes first.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "hrfd_device.h"

#ifndef HRFD_BANK_XCD_ORDER
#define HRFD_BANK_XCD_ORDER 0      /* 1: the mixed bank's WBFM channels on the even XCDs -- MEASURED, NOTHING (profiles/r5_bank_order_ab_NOTHING.txt) */
#endif

namespace hrfd {

// ------------------------------------------------------------------ geometry
struct RxGeometry
{
  bool ragged;                 // the call runs on k_rx_ragged (any block length)
  uint32_t n256;               // 256 kS/s samples per block
  int warm_tiles, seed_terms;  // RxParams of the same names
  int ntiles, origin, hal;
};

// Lengths.  The reference takes any byteCount (IqDataProcessor.cc:926, DataConsumer.cc:229-241: short transfers are
// passed on); what it cannot take is refused here: more than its fixed arrays hold (DataConsumer clips to 262144
// before the call, DataConsumer.cc:229-233; the demodulators' members hold 32768 bytes) and odd counts (its Q loop
// then reads bufferPtr[byteCount], IqDataProcessor.cc:474: the caller rounds up, as hrfd_shim.cc does).
// `warm` is the handle's warm-up knob (kWarm = default), `offgrid` whether the handle has left the grid.
inline int rx_geometry(uint32_t block_bytes, uint32_t n_blocks, uint64_t channel_stride, uint32_t out_b0, uint32_t out_blocks,
                       int serial, int src256, bool offgrid, int warm, RxGeometry *g)
{
  const uint32_t max_bytes = src256 ? 32768u : HRFD_BLOCK_BYTES;
  if (block_bytes == 0 || (block_bytes & 1u) != 0 || block_bytes > max_bytes)
  {
    return fail(HRFD_EINVAL, "%s must be even, > 0 and <= %u (got %u)", src256 ? "bytes_per_channel" : "block_bytes",
                max_bytes, block_bytes);
  }
  // the streaming kernels take whole 1 KiB chunks (inner API: 128 bytes) on a handle that never left the grid
  g->ragged = offgrid || (block_bytes % (src256 ? 128u : 1024u)) != 0;
  if (n_blocks == 0 || out_b0 + n_blocks > out_blocks)
  {
    return fail(HRFD_EINVAL, "bad block count");
  }
  if (channel_stride < (uint64_t)block_bytes * n_blocks)
  {
    return fail(HRFD_EINVAL, "channel_stride smaller than n_blocks*block_bytes");
  }
  if ((uint64_t)block_bytes * n_blocks > 0x7fffffffull)
  {
    // the kernels address a channel's input through a 32-bit buffer descriptor (num_records, byte offsets)
    return fail(HRFD_EINVAL, "n_blocks*block_bytes = %llu exceeds 2^31 - 1 bytes per channel and call",
                (unsigned long long)block_bytes * n_blocks);
  }
  g->n256 = src256 ? block_bytes / 2 : block_bytes / 16;
  const uint32_t halo_unit = src256 ? 2u : 16u;   // input bytes per 256 kS/s sample
  // De-emphasis tiles of kTile samples end at n256.  A lane starts warm_tiles tiles early from a
  // seed summed over seed_terms tiles, so in a block that has to re-derive its history (the first
  // block of a workgroup's run when b > 0) the first `sac` tiles cannot be started properly: they
  // are sacrificial, and tile `sac` must begin at or before the cross-block check position
  // -(kNeedHist + 1), the first sample the integer stages' history is built from.
  g->warm_tiles = (warm >= kWarm) ? kWarmTiles : (warm / 128 < kWarmTiles ? warm / 128 : kWarmTiles);
  g->seed_terms = (warm >= kWarm) ? kSeedTerms : 0;
  const int sac = g->warm_tiles + g->seed_terms;
  g->ntiles = ((int)g->n256 + kNeedHist + 1 + kTile - 1) / kTile + sac;
  g->origin = (int)g->n256 - g->ntiles * kTile;
  g->hal = (-g->origin + 63) / 64 * 64;
  if (!g->ragged && g->ntiles > kMaxTiles)
  {
    return fail(HRFD_EINVAL, "internal: %d de-emphasis tiles exceed %d", g->ntiles, kMaxTiles);
  }
  if (!g->ragged && g->hal > kMaxHal)
  {
    return fail(HRFD_EINVAL, "internal: history %d exceeds %d", g->hal, kMaxHal);
  }
  if (!g->ragged && n_blocks > 1 && (uint32_t)(g->hal + 64) * halo_unit > block_bytes)
  {
    return fail(HRFD_EINVAL, "blocks of %u bytes are too short for a multi-block call "
                "(need >= %u); submit them one per call", block_bytes, (uint32_t)(g->hal + 64) * halo_unit);
  }
  if (serial && n_blocks != 1)
  {
    return fail(HRFD_ESTATE, "internal: serial replay needs n_blocks == 1");
  }
  return HRFD_OK;
}

// ------------------------------------------------------------------ channel lists
// Ten lists of channel ids, list l at lists[l * n ..), counts[l] entries each, ids ascending:
//   0 .. 5  the channels of mode l (HRFD_MODE_*)
//   6       the whole bank: every channel that is not WBFM; a subset: the subset itself
//   7       the AM and SSB channels (one launch for both kinds)
//   8       unused
//   9       the whole bank: every channel that has a demodulator (k_rx_flow_bank); a subset: empty (no bank launch)
// is_subset: the lists are restricted to `subset` (ascending ids, n_subset of them, may be none): the replay of failed
// channels.
constexpr int kRxLists = 10;
constexpr int kRxListNotWb = 6, kRxListAmSsb = 7, kRxListBank = 9;

inline void rx_build_lists(const ChanCfg *cfg, uint32_t n, bool is_subset, const uint32_t *subset, uint32_t n_subset,
                           uint32_t *lists, uint32_t counts[kRxLists])
{
  for (int l = 0; l < kRxLists; l++)
  {
    counts[l] = 0;
  }
  const bool whole = !is_subset;
  const uint32_t members = whole ? n : n_subset;
  for (uint32_t i = 0; i < members; i++)
  {
    const uint32_t c = whole ? i : subset[i];
    const int m = cfg[c].mode;
    // the two rows that differ between the whole bank and a subset are 6 and 9
    const bool in_list[kRxLists] = {m == 0, m == 1, m == 2, m == 3, m == 4, m == 5,
                                    whole ? m != HRFD_MODE_WBFM : true,
                                    m == HRFD_MODE_AM || m == HRFD_MODE_LSB || m == HRFD_MODE_USB,
                                    false,
                                    whole ? m != HRFD_MODE_NONE : false};
    for (int l = 0; l < kRxLists; l++)
    {
      if (in_list[l])
      {
        lists[(size_t)l * n + counts[l]++] = c;
      }
    }
  }
  // List 9 runs as ONE launch, position p on XCD p % 8 (map_unit), a workgroup per channel; the workgroups on the XCDs
  // with odd numbers are 3-5 % slower than the others in most launches (profiles/r5_xcd_swap_experiment.txt) and in the
  // mixed bank the WBFM workgroups end ~10 us behind the FIR kinds'.  -DHRFD_BANK_XCD_ORDER=1 puts the WBFM channels on
  // the even positions: MEASURED AND LEFT OFF -- sixteen WBFM workgroups on an XCD instead of eight run slower by what
  // the placement was to gain (the XCDs' clocks are managed one by one), the bank takes the same time
  // (profiles/r5_bank_order_ab_NOTHING.txt).  Which position a channel has changes nothing it computes.
  if (HRFD_BANK_XCD_ORDER && whole)
  {
    uint32_t *const bank = lists + (size_t)kRxListBank * n;
    std::vector<uint32_t> heavy, light;
    for (uint32_t i = 0; i < counts[kRxListBank]; i++)
    {
      (cfg[bank[i]].mode == HRFD_MODE_WBFM ? heavy : light).push_back(bank[i]);
    }
    size_t ih = 0, il = 0;
    for (uint32_t p = 0; p < counts[kRxListBank]; p++)
    {
      const bool want_heavy = (p & 1u) == 0u;
      const bool take_heavy = (want_heavy && ih < heavy.size()) || il >= light.size();
      bank[p] = take_heavy ? heavy[ih++] : light[il++];
    }
  }
}

// the highest squelch threshold among the channels with a demodulator (can a gate close at all?)
inline int32_t rx_max_threshold(const ChanCfg *cfg, uint32_t n)
{
  int32_t t = INT32_MIN;
  for (uint32_t c = 0; c < n; c++)
  {
    if (cfg[c].mode != HRFD_MODE_NONE && cfg[c].threshold > t)
    {
      t = cfg[c].threshold;
    }
  }
  return t;
}

// The detector's table: 20 log10(i) truncated, entry 0 as entry 1 (DbfsCalculator.cc:58-65); 257 entries.  The kernels
// look a block's mean magnitude (at most 127: a 7-bit full scale) up in it and take 42 and the gain off.
inline void rx_build_dbfs(int32_t *out)
{
  for (int i = 1; i <= 256; i++)
  {
    const float db = 20 * log10f((float)i);
    out[i] = (int32_t)db;
  }
  out[0] = out[1];
}

// Can anybody see the block magnitudes of a launch?  Not when the caller passed no buffer for them AND no gate of the
// bank can close: the detector's lowest level is 0 - 42 - gain_db dBFS, every block is `present` whatever its sum is, and
// PCM, n_pcm, signal_allowed and the committed state follow from the present bits alone.  The comparison is rx_plan's own
// for `gated` -- in 64 bits, so that a gain at which the kernels' 32-bit subtraction wraps counts as "a gate can close" --
// without the gated_pass knob and the 64-block clause: a handle whose gated pass is switched off still needs its sums
// when a gate can close (the channel fails on them and is replayed).
inline bool rx_magnitude_unobservable(int32_t max_threshold, uint32_t gain_db, bool caller_wants_magnitude)
{
  return !caller_wants_magnitude && !((int64_t)max_threshold > -42 - (int64_t)gain_db);
}

// ------------------------------------------------------------------ the plan
// one value per kernel instantiation a receive launch starts (k_rx_ragged has no plan: rx_launch takes that path before)
enum RxKernel : uint8_t
{
  kRxFlowBank, kRxFlowBankDump,          // k_rx_flow_bank<SVC, DUMP>
  kRxFlowAs, kRxFlowAsDump,              // k_rx_wbfm_flow<SVC, false, DUMP, 14>
  kRxFlowFm, kRxFlowFmDump,              // k_rx_wbfm_flow<SVC, false, DUMP, 2>
  kRxFlowWb, kRxFlowWbDump,              // k_rx_wbfm_flow<SVC, false, DUMP>
  kRxGatedWb, kRxGatedFm, kRxGatedAs,    // k_rx_wbfm_flow<SVC, true, false, 3 | 2 | 14>
  kRxFirAs, kRxFirAs256,                 // k_rx_fir<14, S256, false>
  kRxPostAs,                             // k_rx_post<14>
  kRxFirFm, kRxFirFm256, kRxFirFmArith,  // k_rx_fir<2, S256, ARITH>
  kRxBlocksNone,                         // k_rx_wbfm<0, false, false>
  kRxBlocksWb, kRxBlocksWb256, kRxBlocksWbArith,   // k_rx_wbfm<3, S256, ARITH>
  kRxFinish,                             // k_rx_finish
  kRxKernels
};

struct RxStep
{
  uint8_t kernel;              // RxKernel
  int8_t list;                 // the channel list it runs over; -1 (k_rx_finish only): channels 0 .. n_list - 1
  uint32_t n_list;
  uint32_t grid, block;
  uint32_t run_len, n_runs;    // RxParams of the same names
  int32_t warm_tiles;
  bool self_finish;            // the kernel finishes its channels itself (finish_channel)
  bool dbg;                    // the phase-stamp buffer is attached
  bool expire_once;            // this launch consumes the pending hrfd_rx_debug_expire
};

// At most 11: k_rx_fir + k_rx_post and k_rx_fir for the FIR kinds, the WBFM flow kernel with its gated launch, mode NONE,
// and k_rx_finish for the five modes that did not finish themselves (a FIR kind on a flow kernel means 48 channels, and
// with a second kind the bank launch).  tests/cpp/san_rx_plan.cc walks the whole grid under ASan.
constexpr int kRxMaxSteps = 12;

struct RxPlan
{
  int n;
  RxStep step[kRxMaxSteps];
};

struct RxPlanIn
{
  uint32_t count[kRxLists];    // rx_build_lists
  uint32_t n_channels;         // of the handle
  uint32_t n_blocks, n256;
  uint32_t gain_db;
  int32_t max_threshold;       // rx_max_threshold
  int warm_tiles;              // RxGeometry
  bool serial, src256, subset, dump;   // dump: the iq256 output is wanted
  // the handle's knobs (test hooks)
  int use_stream, atan_mode, fir_flow, gated_pass, run_len;
  bool tab_ok, quad_ok, arith_ok;
  bool has_dbg;                // a phase-stamp buffer of dbg_cap words exists
  size_t dbg_cap;
};

inline uint32_t rx_groups(uint32_t n) { return 8u * ((n + 7u) / 8u); }   // a workgroup per channel, whole rounds of the 8 XCDs

// Everything goes to the caller's stream, in this order of preference:
//  1. k_rx_flow_bank: a bank of several kinds (WBFM, FM, AM / SSB) as ONE launch -- one persistent workgroup per
//     channel, the mode read per workgroup, every channel finished inside (BASELINE config 3);
//  2. k_rx_wbfm_flow<.., MODE> per kind, the same shape, when there are channels enough of that kind to fill the
//     chip that way (WBFM: always; BASELINE configs 2 and 4), behind it the gated pass for WBFM channels whose
//     squelch gates may close;
//  3. the block kernels (one workgroup per channel-block: k_rx_wbfm, k_rx_fir + k_rx_post) with k_rx_finish behind
//     them: single-block calls (the reference's cadence), the inner demodulator API, the exact replay of a subset,
//     block sizes that are not whole units of 512 samples at 256 kS/s, small banks.
// The flow shapes need whole units of two 4 KiB pieces per block, at most 64 blocks, and the first-octant table.
inline RxPlan rx_plan(const RxPlanIn &in)
{
  RxPlan plan;
  plan.n = 0;
  bool expire_pending = true;                              // the first flow launch of a call takes the hook
  auto push = [&](RxKernel k, int list, uint32_t n, uint32_t grid, uint32_t block, uint32_t run_len, uint32_t n_runs) -> RxStep & {
    RxStep &s = plan.step[plan.n++];
    s = RxStep{(uint8_t)k, (int8_t)list, n, grid, block, run_len, n_runs, in.warm_tiles, false, false, false};
    return s;
  };
  const uint32_t n_blocks = in.n_blocks;
  const uint32_t n_wb = in.count[HRFD_MODE_WBFM], n_as = in.count[kRxListAmSsb], n_fm = in.count[HRFD_MODE_FM];
  const bool batch = n_blocks > 1 && !in.serial && !in.src256 && !in.subset;
  // (the flow shapes need their tables: the first-octant one with its corrections -- FM, and the round-4 WBFM build --
  //  and the first-quadrant one of the re-split WBFM chain; both are proven against the reference table at create)
  const bool flow_shape = batch && in.use_stream == 2 && in.tab_ok && (HRFD_FLOW_SPLIT == 0 || in.quad_ok) && in.atan_mode != 0 &&
                          (in.n256 % 512u) == 0 && in.n256 >= 2048u;
  const bool fir_shape = flow_shape && in.fir_flow != 0 && n_blocks <= 64u;
  const int kinds = (n_wb != 0) + (n_as != 0) + (n_fm != 0);
  const bool bank = fir_shape && kinds >= 2 && in.fir_flow != 2 && (in.fir_flow > 0 || in.count[kRxListBank] >= 48u);
  // which kinds run on a flow kernel, and so finish their own channels
  const bool wb_flow = bank || (flow_shape && n_wb != 0);
  const bool as_flow = bank || (fir_shape && n_as != 0 && (in.fir_flow > 0 || n_as >= 48u));
  const bool fm_flow = bank || (fir_shape && n_fm != 0 && (in.fir_flow > 0 || n_fm >= 48u));
  // Squelch (Squelch.cc:227-273, IqDataProcessor.cc:961-1034).  The detector's lowest level is 0 - 42 - gain_db dBFS
  // (DbfsCalculator.cc:111-147): with a threshold at or below it -- the reference's default is -200 -- no gate of
  // the bank can ever close and the batch launch is all there is.  Otherwise the gated pass follows, one launch per
  // kind: its workgroups redo the channels that failed on a closed gate, exactly, and the others leave at once.
  const bool gated = in.gated_pass && n_blocks <= 64u && (int64_t)in.max_threshold > -42 - (int64_t)in.gain_db;
  const bool arith = in.arith_ok && in.atan_mode != 0;     // theta computed instead of gathered from the table

  // k_rx_wbfm_flow / k_rx_flow_bank over a channel list: one run per channel unless the WBFM bank alone is too small
  // to fill the chip with whole-CU workgroups
  auto flow = [&](RxKernel k, int list, uint32_t n, bool wbfm_runs) {
    const uint32_t groups = rx_groups(n);
    uint32_t run_len = n_blocks;
    if (wbfm_runs)
    {
      // runs of consecutive blocks per workgroup (only a run's first block re-produces the history in front of it):
      // as long as possible while the launch still fills the chip -- up to the 64 blocks a workgroup can finish from LDS
      // (round 5; rounds 2-4 stopped at 16: a 64-block batch of 256 channels was four runs per channel, each with its own
      // table copy, re-derived history and service tail -- `also.wbfm_256x64` of the bench line)
      run_len = (in.run_len > 0) ? (uint32_t)in.run_len : 64u;
      run_len = run_len < n_blocks ? run_len : n_blocks;
      while (in.run_len <= 0 && run_len > 1 && groups * ((n_blocks + run_len - 1) / run_len) < 256u)
      {
        run_len--;
      }
    }
    const uint32_t n_runs = (n_blocks + run_len - 1) / run_len;
    // (`enable iqdump`: the 256 kS/s stream goes out of the stream waves as well -- the DUMP instantiation is the next id)
    RxStep &s = push((RxKernel)(k + (in.dump ? 1 : 0)), list, n, groups * n_runs, kThreads, run_len, n_runs);
    s.dbg = in.has_dbg && (size_t)s.grid * kDbgSlots <= in.dbg_cap;   // (probe builds: one launch per call -- one mode, or the bank)
    s.warm_tiles = in.warm_tiles < HRFD_FLOW_WARM_TILES ? in.warm_tiles : HRFD_FLOW_WARM_TILES;   // tiles of 64 here (the FIR modes: ring tiles read below a generation)
    s.self_finish = true;                                  // the last workgroup of a channel finishes it (finish_channel)
    s.expire_once = expire_pending;
    expire_pending = false;
  };
  auto gated_flow = [&](RxKernel k, int list, uint32_t n) {
    if (gated && n != 0)
    {
      RxStep &s = push(k, list, n, rx_groups(n), kThreads, n_blocks, 1);
      s.warm_tiles = in.warm_tiles < HRFD_FLOW_WARM_TILES ? in.warm_tiles : HRFD_FLOW_WARM_TILES;
      s.self_finish = true;
    }
  };
  // the block kernels of mode NONE (front end and squelch only) and WBFM: runs of blocks per workgroup
  auto blocks = [&](RxKernel k, int list) {
    const uint32_t n = in.count[list], groups = rx_groups(n);
    uint32_t run_len = (in.run_len > 0) ? (uint32_t)in.run_len : 8u;
    run_len = run_len < n_blocks ? run_len : n_blocks;
    while (in.run_len <= 0 && run_len > 1 && groups * ((n_blocks + run_len - 1) / run_len) < 512u)
    {
      run_len--;
    }
    if (in.serial || in.src256)
    {
      run_len = 1;
    }
    const uint32_t n_runs = (n_blocks + run_len - 1) / run_len;
    RxStep &s = push(k, list, n, groups * n_runs, kThreads, run_len, n_runs);
    s.dbg = in.has_dbg && (size_t)s.grid * kDbgSlots <= in.dbg_cap && list == HRFD_MODE_WBFM;
  };
  // k_rx_fir: a workgroup per channel-block
  auto fir = [&](RxKernel k, int list, uint32_t n) { push(k, list, n, rx_groups(n) * n_blocks, kThreads, 1, n_blocks); };

  if (bank)
  {
    flow(kRxFlowBank, kRxListBank, in.count[kRxListBank], false);
    gated_flow(kRxGatedWb, HRFD_MODE_WBFM, n_wb);
    gated_flow(kRxGatedFm, HRFD_MODE_FM, n_fm);
    gated_flow(kRxGatedAs, kRxListAmSsb, n_as);
  }
  else
  {
    // AM and SSB: one launch for both kinds (the same three decimators), then their 8 kS/s recurrences
    if (as_flow)
    {
      flow(kRxFlowAs, kRxListAmSsb, n_as, false);
      gated_flow(kRxGatedAs, kRxListAmSsb, n_as);
    }
    else if (n_as != 0)
    {
      fir(in.src256 ? kRxFirAs256 : kRxFirAs, kRxListAmSsb, n_as);
      push(kRxPostAs, kRxListAmSsb, n_as, n_as, 256, 1, n_blocks);
    }
    if (fm_flow)
    {
      flow(kRxFlowFm, HRFD_MODE_FM, n_fm, false);
      gated_flow(kRxGatedFm, HRFD_MODE_FM, n_fm);
    }
    else if (n_fm != 0)
    {
      fir(in.src256 ? kRxFirFm256 : arith ? kRxFirFmArith : kRxFirFm, HRFD_MODE_FM, n_fm);
    }
    if (wb_flow)
    {
      flow(kRxFlowWb, HRFD_MODE_WBFM, n_wb, true);
      gated_flow(kRxGatedWb, HRFD_MODE_WBFM, n_wb);
    }
    else if (n_wb != 0)
    {
      blocks(in.src256 ? kRxBlocksWb256 : arith ? kRxBlocksWbArith : kRxBlocksWb, HRFD_MODE_WBFM);
    }
  }
  if (in.count[HRFD_MODE_NONE] != 0)
  {
    blocks(kRxBlocksNone, HRFD_MODE_NONE);
  }
  // the channels that no kernel finished by itself
  auto finish = [&](int list, uint32_t n) {
    if (n != 0)
    {
      push(kRxFinish, list, n, n, 64, 1, n_blocks);
    }
  };
  if (in.subset)
  {
    finish(kRxListNotWb, in.count[kRxListNotWb]);          // the subset itself
  }
  else if (!wb_flow && !as_flow && !fm_flow)
  {
    finish(-1, in.n_channels);                             // everything, one launch
  }
  else
  {
    const bool self[6] = {false, as_flow, fm_flow, wb_flow, as_flow, as_flow};   // by HRFD_MODE_*
    for (int m = 0; m < 6; m++)
    {
      if (!self[m])
      {
        finish(m, in.count[m]);
      }
    }
  }
  return plan;
}

} // namespace hrfd
