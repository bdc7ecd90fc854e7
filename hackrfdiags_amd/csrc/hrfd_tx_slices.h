// hackrfdiags_amd/csrc/hrfd_tx_slices.h -- what a modulator launch (hrfd_mod_process_device, hrfd_api_tx.hip) decides
// before it touches the device: the refusal of calls whose 32-bit arithmetic would wrap, the time slices of the WBFM and
// FM modulators, the grids of every pass and the choice of the phase recurrence's kernel.  Pure functions: no HIP call, no
// handle, no allocation.  Plain C++ (tests/cpp/san_tx_slices.cc compiles it on the CPU and tests/tx_slices_model.py
// states the same rules a second time); the includer declares `int fail(int code, const char *fmt, ...)` and the HRFD_*
// codes first.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef HRFD_MOD_TILE
#define HRFD_MOD_TILE 128          /* hrfd_tx_kernels.hip: input samples per k_mod workgroup */
#endif
#ifndef HRFD_PHASE_ROWS8
#define HRFD_PHASE_ROWS8 1         /* 0: k_phase_rows (four steps per lane) where k_phase_rows8 would run (A/B switch) */
#endif

namespace hrfd {

// the kernels' shapes (hrfd_tx_kernels.hip; hrfd_api_tx.hip asserts that they are the kernels' own)
constexpr uint32_t kTxTile = HRFD_MOD_TILE, kTxModThreads = 256;
constexpr uint32_t kTxWtRun = 2048, kTxWtThreads = 1024, kTxWbRailsThreads = 512;
constexpr uint32_t kTxUnit = 64;           // the slices' lengths are in units of 64 input samples, whatever the cascade's tile
constexpr int kTxMaxSlices = 32;           // of a WBFM call: the handle holds an event pair per slice
static_assert(kTxTile == 64 || kTxTile == 128, "the cuts below fall on multiples of 128 samples: whole tiles");

// ------------------------------------------------------------------ the refusal
// A call of n samples for each of C channels is accepted when none of the following wraps.
//  1. Every kind ends in k_mod over the whole call or over slices of it: 8 ceil(C / 8) * ceil(n / kTxTile) workgroups of
//     kTxModThreads threads at most, and gridDim.x * blockDim.x has to fit 32 bits (bank_check_call's rule): at most
//     (2^32 - 1) / 256 = 2^24 - 1 workgroups, counted here in 64 bits.  That bound carries the others of the launchers:
//       * at least 8 workgroups per tile, so n <= 128 (2^21 - 1) < 2^28: (n + 127) / 128, (n + 63) / 64, (int)n and k_mod's
//         tile * kModTile in int cannot wrap, and no slice has more tiles than the call;
//       * C n <= 128 * workgroups < 2^31: the baseband passes' ceil(C n / 256) workgroups (k_am_rails, k_fm_step,
//         k_fm_rails, k_sig_rails) stay below 2^23, k_wb_rails' ceil(len / 64) C work items and k_wb_tail's
//         ceil(C / 8) ceil(len / 64) below 2^25;
//       * C <= 2^24 - 1: (C + 7) / 8, (C + 15) / 16 and (C + 63) / 64 (the recurrences, k_sig_fm) cannot wrap.
//  2. The WBFM modulator indexes 32 n cells per channel: k_wb_tail and k_wb_rails in uint32_t (n32 = n * 32u and up to
//     512 cells beyond it), k_mod<WB_TAIL> in int (g = 32 t0 + t - 2 with t0 < n and t < 2 + 32 kTxTile).  So
//     32 n + 32 kTxTile <= 2^31 - 1.  (k_phase_rows' 32-bit byte offset is the launcher's own choice: tx_scan_kernel.)
// hrfd_duc_transmit's calls (n <= 65536, C <= 32768, C n / 4 workgroups of its own within the same 2^24 - 1) all pass.
constexpr uint64_t kTxMaxWgs = 0xffffffffull / kTxModThreads;
constexpr uint32_t kTxWbfmMaxN = 0x7fffffffu / 32u - kTxTile;

inline uint64_t tx_mod_wgs(uint32_t n_channels, uint32_t n)
{
  return 8u * (((uint64_t)n_channels + 7u) / 8u) * (((uint64_t)n + kTxTile - 1u) / kTxTile);
}

inline int tx_check_call(const char *who, int kind, uint32_t n_channels, uint32_t n_per_channel)
{
  if (tx_mod_wgs(n_channels, n_per_channel) > kTxMaxWgs)
  {
    return fail(HRFD_EINVAL, "%s: %u channels x %u samples need %llu workgroups, more than the %llu one launch takes", who,
                n_channels, n_per_channel, (unsigned long long)tx_mod_wgs(n_channels, n_per_channel),
                (unsigned long long)kTxMaxWgs);
  }
  if (kind == HRFD_MOD_WBFM && n_per_channel > kTxWbfmMaxN)
  {
    return fail(HRFD_EINVAL, "%s: %u channels x %u samples: the WBFM modulator's 32 cells per sample take at most %u samples "
                "per channel (32-bit indices)", who, n_channels, n_per_channel, kTxWbfmMaxN);
  }
  return HRFD_OK;
}

// ------------------------------------------------------------------ time slices
inline uint32_t tx_units(uint32_t n) { return (n + kTxUnit - 1u) / kTxUnit; }

// The WBFM modulator's passes run in TIME SLICES of the call, the phase recurrence of slice t + 1 beside the lookup and the
// x8 cascade of slice t (mod_launch_wbfm).  A call is cut when it has more than 24 units, counted even (the last slice ends
// with the call whatever is left) -- apart from what the handle knows: its hook, its streams.
inline uint32_t tx_wbfm_units(uint32_t n) { return tx_units(n) & ~1u; }
inline bool tx_wbfm_sliceable(uint32_t n) { return tx_wbfm_units(n) > 24u; }

// out[k]: the end of slice k in input samples; the count is returned (1: the whole call).  The recurrence takes ~0.54 us
// per input sample, a head pass ~0.1, rails and tail together ~0.25 (on the CUs the recurrence leaves them) plus ~30 us of
// launches: slices may grow fourfold at the start (the next head pass is through before the recurrence of the slice in
// front is) and halve at the end (a slice's rails and tail are through before the next, shorter recurrence is); what stays
// exposed is the first slice's head pass and the last slice's rails and tail, so those two slices are two units long.
// Every slice costs the recurrence a launch (~20 us): long pieces between, even shares of at least 32 units.
// Every length is an even number of units, so a cut is a multiple of 128 samples: a whole tile, and a whole chunk of
// k_phase_rows8's 128 steps x 32.  max_slices >= 8; out holds max_slices entries.
inline int tx_wbfm_cuts(uint32_t n_per_channel, uint32_t max_slices, uint32_t *out)
{
  int n_cuts = 0;
  if (tx_wbfm_sliceable(n_per_channel))
  {
    const uint32_t nt = tx_wbfm_units(n_per_channel);
    uint32_t lo = 0;
    auto cut = [&](uint32_t units) {
      lo += units * kTxUnit;
      out[n_cuts++] = lo;
    };
    static const uint32_t kTail[4] = {16, 8, 4, 2};
    const bool long_tail = nt >= 72u;
    const uint32_t n_tail = long_tail ? 4u : 2u;           // {16, 8, 4, 2} or {4, 2}
    cut(2);
    cut(8);
    uint32_t mid = nt - 10u - (long_tail ? 30u : 6u);
    const uint32_t room = max_slices - 2u - n_tail - 1u;
    const uint32_t piece = 32u > (mid + room - 1u) / room ? 32u : (mid + room - 1u) / room;
    while (mid != 0u)
    {
      const uint32_t k = (mid + piece - 1u) / piece;       // pieces still to go: even shares
      uint32_t len = ((mid + k - 1u) / k + 1u) & ~1u;      // (an even number of units; the last piece takes what is left)
      len = len < mid ? len : mid;
      cut(len);
      mid -= len;
    }
    for (uint32_t k = 4u - n_tail; k < 3u; k++)
    {
      cut(kTail[k]);
    }
  }
  out[n_cuts++] = n_per_channel;                           // (the last slice ends with the call, whole tile or not)
  return n_cuts;
}

// The FM modulator cuts a call of 64 units or more into three slices: the recurrence + cos / sin of a slice take ~1.9 us
// per unit, the cascade ~5.9: a slice may be three times the one in front (mod_launch_fm).  out: 0, two cuts on even units
// (whole tiles of 64 or 128), n_per_channel.
inline bool tx_fm_sliceable(uint32_t n) { return tx_units(n) >= 64u; }

inline void tx_fm_cuts(uint32_t n_per_channel, uint32_t out[4])
{
  const uint32_t nt = tx_units(n_per_channel);
  const uint32_t l0 = ((8u > nt / 16u ? 8u : nt / 16u) + 1u) & ~1u;
  const uint32_t l1 = (3u * l0 + l0 / 2u < nt - l0 - 2u ? 3u * l0 + l0 / 2u : nt - l0 - 2u) & ~1u;
  out[0] = 0u;
  out[1] = l0 * kTxUnit;
  out[2] = (l0 + l1) * kTxUnit;
  out[3] = n_per_channel;
}

// ------------------------------------------------------------------ grids
// k_mod over `len` samples of every channel: channels are dealt to the 8 XCDs in whole groups of eight, a workgroup per tile
inline uint32_t tx_groups8(uint32_t n_channels) { return 8u * ((n_channels + 7u) / 8u); }
inline uint32_t tx_tiles(uint32_t len) { return (len + kTxTile - 1u) / kTxTile; }
inline uint32_t tx_mod_grid(uint32_t n_channels, uint32_t len) { return tx_groups8(n_channels) * tx_tiles(len); }

// the baseband passes: a thread per sample, 256 per workgroup
inline uint32_t tx_base_grid(uint32_t n_channels, uint32_t len) { return (uint32_t)(((uint64_t)len * n_channels + 255u) / 256u); }

// k_wb_tail over `span` samples of every channel: persistent workgroups, eight XCDs' worth, a wave per work item of kTxWtRun cells
inline uint32_t tx_wb_tail_grid(uint32_t n_channels, uint32_t span, uint32_t max_wgs)
{
  const uint32_t runs = (span * 32u + kTxWtRun - 1u) / kTxWtRun;
  const uint32_t items_x = ((n_channels + 7u) / 8u) * runs;          // work items of the fullest XCD
  const uint32_t waves = kTxWtThreads / 64u;
  const uint32_t want = (items_x + waves - 1u) / waves, most = max_wgs / 8u;
  const uint32_t wgs_x = want < most ? want : most;
  return 8u * (wgs_x > 1u ? wgs_x : 1u);
}

// k_wb_rails: four cells per thread
inline uint32_t tx_wb_rails_grid(uint32_t n_channels, uint32_t span, uint32_t max_wgs)
{
  const uint64_t q = (uint64_t)span * 32u / 4u * n_channels;
  const uint64_t want = (q + kTxWbRailsThreads - 1u) / kTxWbRailsThreads;
  return (uint32_t)(want < max_wgs ? want : max_wgs);
}

// The Nco phase recurrence over `steps` cells per channel, rows `row_stride` cells apart: k_phase_rows (four channels per
// wave, a lone wave per SIMD up to 4096 channels, two up to 8192: the wave's time per step is the same; whole chunks of 64
// steps, which every call and every time slice is, and 4 * row_stride within a 32-bit byte offset) -- eight steps per lane
// where the step count allows whole chunks of 128, every WBFM call and time slice (round 6); banks beyond that put more waves
// on a SIMD than that shape likes and keep round 2's k_phase_scan<64> (64 channels per recurrence wave), which takes whole
// quads of cells; anything else runs on the plain kernel.  scan_kind is the handle's test hook: 1 = never k_phase_rows,
// 2 = k_phase_rows where k_phase_rows8 would run.
enum TxScan : uint8_t { kTxScanRows8, kTxScanRows, kTxScan64, kTxScanPlain };

inline TxScan tx_scan_kernel(int scan_kind, uint32_t n_channels, uint64_t steps, uint64_t row_stride)
{
  if (scan_kind != 1 && n_channels <= 8192u && (steps & 63u) == 0 && row_stride < (1ull << 28))
  {
    return (scan_kind != 2 && HRFD_PHASE_ROWS8 && (steps & 127u) == 0) ? kTxScanRows8 : kTxScanRows;
  }
  return ((steps & 3u) == 0 && (row_stride & 3u) == 0) ? kTxScan64 : kTxScanPlain;
}

inline uint32_t tx_scan_grid(TxScan k, uint32_t n_channels)
{
  return (k == kTxScanRows8 || k == kTxScanRows) ? (n_channels + 15u) / 16u : (n_channels + 63u) / 64u;
}

} // namespace hrfd
