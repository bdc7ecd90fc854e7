// hackrfdiags_amd/csrc/hrfd_dcs.hip -- hrfd_dcs_*: digital coded squelch decoded on the receive chain's PCM.
//
// PCM rows [C][n_blocks][512] int16 (and n_pcm) in; per block the count of samples whose 23-bit word is each listed code
// (hits), and the tone bank's kind of verdict over them (best, present).  Exact integer arithmetic, contract in
// include/hrfd.h; tests/dcs_model.py restates it in numpy, hrfd_dcs.h holds the laws both sides of this file share.
//
// k_dcs: ONE pass, one workgroup of 256 threads per channel, which walks its row in tiles of kDcsTile = 4 blocks: 8
// consecutive samples per lane, so wave w of the workgroup has block w of the tile to itself from the filter to the verdict.
//   A. the tile's samples and the 512 in front of them go into LDS exactly as k_audio_fir lays them (zero behind each
//      block's n_pcm; the handle's state in front of block 0, the block before under its own n_pcm in front of a later tile),
//      and the filter is k_audio_fir's: audio_fir_run, taps through the scalar cache, three ds_read_b128 and 64
//      v_dot2_i32_i16 a step.  Only acc > 0 leaves it: a lane's 8 signs are one byte of a bit array in LDS, which holds the
//      1312 slicer bits in front of the tile (41 dwords) and the tile's 2048 behind them (a lane owns a whole byte, so the
//      store needs no ballot)
//   B. bit k of the words of a lane's 8 samples are 8 neighbouring bits of that array, D[k] in front of the lane's byte: two
//      ds_read_b32 and one v_alignbit_b32 give them (lanes 8 bits apart: four lanes share a dword, a wave reads 17
//      neighbouring dwords, no bank conflict), so 23 such reads serve 8 samples.  The 8 words are put together bit by bit;
//      the least of the 23 rotations of each is one v_alignbit_b32 and one v_min_u32 a rotation over the word repeated
//      three times, with the rotation in the upper 23 bits (the lower 9 decide ties between equal rotations only); a
//      binary search over the sorted list of canonical words in LDS (7 steps, padded to 128) names the entry.  The wave
//      counts: for every entry some lane matched, a ballot and a popcount, added in the lane that keeps the entry's counter
//      (entry e in lane e & 63, counter e >> 6): no LDS or global atomics, and no counter is shared between waves
//   C. the block's K counts go out as dwords where the row of hits is 4-byte aligned (two shuffles pair neighbouring
//      entries), as halfwords where it is not; best and present come out of four max-reductions over (hits << 8 | 255 - k)
//   After the last tile the last block as the filter saw it and the last 1312 slicer bits go to the other side of the state.
// Between tiles the bit array moves down by the tile's 64 dwords through registers.  Four barriers a tile.
// The grid is the channel count, at most 65536 workgroups: below kBankMaxWgs, so the launch is never cut (as k_level's).
// No float, no atomics; every result leaves through a vector store.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "hrfd_dcs.h"

namespace hrfd {

constexpr int kDcsThreads = 256;
constexpr int kDcsTile = 4;                                // blocks of one tile
constexpr int kDcsPer = 8;                                 // consecutive samples of one lane
constexpr int kDcsXsDw = 4 + (kDcsTile + 1) * (int)kDcsHistDw + 12;      // k_audio_fir's: offset, history, tile, the last step's reach
constexpr int kDcsTileBitDw = kDcsTile * (int)kDcsBlock / 32;           // 64
constexpr int kDcsBitsDw = ((int)kDcsBitDw + kDcsTileBitDw + 1 + 3) / 4 * 4;      // history, tile, the dword above the newest byte
static_assert(kDcsTile == kAudioRun && kDcsPer == kAudioPer && kDcsThreads == kAudioThreads && kDcsMaxTaps == kAudioMaxTaps &&
                  kDcsXsDw == kAudioXsDw,
              "stage A is k_audio_fir's layout and audio_fir_run");
static_assert(kDcsTile * (int)kDcsBlock == kDcsThreads * kDcsPer && (int)kDcsBlock == 64 * kDcsPer, "a wave has one block of the tile");
static_assert(kDcsBitHist >= kDcsReach && kDcsBitHist % 8 == 0, "a lane's byte lies on a byte of the bit array");
static_assert(kDcsMaxCodes == 128, "two counters a lane, and a search of 7 steps");
static_assert(16 * ((kDcsXsDw + 3) / 4) + 4 * kDcsBitsDw + 5 * (int)kDcsMaxCodes <= 8192, "LDS: 8 KiB a workgroup, so eight fit a CU beside others");
static_assert(65536u <= kBankMaxWgs, "one workgroup per channel is one launch");

// what k_dcs reads of the code list: the canonical words in rising order (kDcsNoEntry behind the K-th) with the entry of
// each, the group of every entry in list order, the thresholds
struct DcsList
{
  uint32_t sorted[kDcsMaxCodes];
  uint8_t entry[kDcsMaxCodes];
  uint8_t group[kDcsMaxCodes];
  uint32_t min_hits[kDcsGroups];
};

struct DcsParams
{
  const int16_t *pcm;                      // [C] rows of n_blocks x 512 samples, stride bytes apart, even address
  uint64_t stride;
  const uint32_t *n_pcm;                   // [C][n_blocks] or NULL
  const uint32_t *state_in;                // [C][kDcsStateDw]
  uint32_t *state_out;
  const uint8_t *reset;                    // [C]: non-zero = this channel starts from zeros; or NULL
  uint16_t *hits;                          // [C][n_blocks][K] at an even address, or NULL
  uint8_t *best, *present;                 // [C][n_blocks][4], or NULL
  uint32_t n_blocks, T, J, K;
};

// rule 4 on the device: ww = w repeated from bit 0, 23 and 46; bits r + 9 .. r + 31 of it are a rotation of w for every r,
// and r = 0..22 gives all 23
__device__ __forceinline__ uint32_t dcs_canonical_fast(uint32_t w)
{
  const uint32_t lo = w | (w << 23), hi = (w >> 9) | (w << 14);
  uint32_t m = lo;
#pragma unroll
  for (uint32_t r = 1; r < kDcsWordBits; r++)
  {
    m = min(m, __builtin_amdgcn_alignbit(hi, lo, r));
  }
  return m >> 9;
}

// taps: [P.J] (even, odd) pairs, J a multiple of kAudioStep; list: the handle's; parameters of their own so that they can
// be __restrict__ and come through the scalar cache
__global__ __launch_bounds__(kDcsThreads) void k_dcs(const DcsParams P, const uint2 *__restrict__ taps, const DcsList *__restrict__ list)
{
  __shared__ audio_u4 xs4[(kDcsXsDw + 3) / 4];
  __shared__ uint32_t bits[kDcsBitsDw];
  __shared__ uint32_t sorted[kDcsMaxCodes];
  __shared__ uint8_t entry[kDcsMaxCodes];
  uint32_t *xs = (uint32_t *)xs4;
  const uint32_t tid = threadIdx.x, c = blockIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t par = (P.T - 1) & 1u, lead = (kDcsBlock + 1 - P.T - par) / 2, pad = (4u - (lead & 3u)) & 3u;
  const int16_t *row = (const int16_t *)((const char *)P.pcm + (uint64_t)c * P.stride);
  const uint32_t *n_row = P.n_pcm != nullptr ? P.n_pcm + (uint64_t)c * P.n_blocks : nullptr;
  const bool fresh = P.reset != nullptr && P.reset[c] != 0;
  const uint32_t *st_in = P.state_in + (uint64_t)c * kDcsStateDw;
  uint32_t *st_out = P.state_out + (uint64_t)c * kDcsStateDw;

  if (tid < kDcsMaxCodes)
  {
    sorted[tid] = list->sorted[tid];
    entry[tid] = list->entry[tid];
  }
  if (tid < (uint32_t)kDcsBitsDw)
  {
    bits[tid] = tid < kDcsBitDw && !fresh ? st_in[kDcsHistDw + tid] : 0u;
  }
  // the groups of the two entries whose counters this lane keeps
  const uint32_t grp0 = lane < P.K ? list->group[lane] : kDcsGroups, grp1 = 64 + lane < P.K ? list->group[64 + lane] : kDcsGroups;

  for (uint32_t b0 = 0; b0 < P.n_blocks; b0 += kDcsTile)
  {
    const uint32_t nb = min((uint32_t)kDcsTile, P.n_blocks - b0);
    const bool last = b0 + nb == P.n_blocks;
    const bool active = wave < nb;                         // the wave's block lies in the row

    // A. the samples: dword idx holds samples 2 idx - 512 and 2 idx - 511 of the tile
    for (uint32_t idx = tid; idx < (uint32_t)kDcsXsDw - pad; idx += kDcsThreads)
    {
      const uint32_t blk = idx / kDcsHistDw, j = idx - blk * kDcsHistDw;
      uint32_t d = 0;
      if (blk == 0 && b0 == 0)
      {
        d = fresh ? 0u : st_in[j];
      }
      else if (blk <= nb)
      {
        const uint32_t sb = b0 + blk - 1, lim = pcm_block_limit(n_row, sb), pos = 2 * j;
        if (pos < lim)
        {
          const int16_t *src = row + (uint64_t)sb * kDcsBlock + pos;
          if (((uintptr_t)src & 3u) == 0)
          {
            d = *(const uint32_t *)src;
          }
          else
          {
            d = (uint32_t)(uint16_t)src[0] | ((uint32_t)(uint16_t)src[1] << 16);
          }
          d = pos + 1 < lim ? d : (d & 0xffffu);
        }
      }
      xs[pad + idx] = d;
    }
    __syncthreads();
    if (last)
    {
      st_out[tid] = xs[pad + nb * kDcsHistDw + tid];       // the last block as the filter saw it
    }

    //    the filter and the slicer
    if (active)
    {
      int acc[kDcsPer];
#pragma unroll
      for (int i = 0; i < kDcsPer; i++)
      {
        acc[i] = 0;
      }
      const audio_u4 *win = xs4 + (pad + lead + tid * kDcsPer / 2) / 4;      // 16-byte aligned by the choice of pad
      if (par)
      {
        audio_fir_run<1>(win, taps, P.J, acc);
      }
      else
      {
        audio_fir_run<0>(win, taps, P.J, acc);
      }
      uint32_t sign = 0;
#pragma unroll
      for (int i = 0; i < kDcsPer; i++)
      {
        sign |= (acc[i] > 0 ? 1u : 0u) << i;
      }
      ((uint8_t *)bits)[kDcsBitHist / 8 + tid] = (uint8_t)sign;
    }
    __syncthreads();

    if (active)
    {
      // B. bit k of the lane's 8 words: the 8 bits from D[k] in front of its byte on
      uint32_t col[kDcsWordBits];
#pragma unroll
      for (uint32_t k = 0; k < kDcsWordBits; k++)
      {
        const uint32_t pos = kDcsBitHist + kDcsPer * tid - dcs_delay(k);
        col[k] = __builtin_amdgcn_alignbit(bits[(pos >> 5) + 1], bits[pos >> 5], pos & 31u);
      }
      uint32_t cnt0 = 0, cnt1 = 0;                         // the hits of entries lane and 64 + lane in this block
#pragma unroll
      for (int i = 0; i < kDcsPer; i++)
      {
        uint32_t w = 0;
#pragma unroll
        for (uint32_t k = 0; k < kDcsWordBits; k++)
        {
          w |= ((col[k] >> i) & 1u) << (kDcsWordBits - 1 - k);
        }
        const uint32_t cw = dcs_canonical_fast(w);
        uint32_t at = 0;
#pragma unroll
        for (uint32_t step = kDcsMaxCodes / 2; step != 0; step >>= 1)
        {
          at += sorted[at + step - 1] < cw ? step : 0u;
        }
        const uint32_t e = sorted[at] == cw ? entry[at] : kDcsNoEntry;
        unsigned long long pending = __ballot(e != kDcsNoEntry);
        while (pending != 0)
        {
          const uint32_t which = (uint32_t)__builtin_amdgcn_readlane((int)e, (int)__builtin_ctzll(pending));
          const unsigned long long same = __ballot(e == which);
          pending &= ~same;
          const uint32_t n = (uint32_t)__popcll(same);
          cnt0 += lane == which ? n : 0u;
          cnt1 += lane + 64 == which ? n : 0u;
        }
      }

      // C. the block's outputs
      const uint64_t blk = (uint64_t)c * P.n_blocks + b0 + wave;
      const uint32_t e0 = 2 * lane, from = e0 & 63u;       // this lane stores entries e0 and e0 + 1
      const uint32_t a0 = __shfl(cnt0, from), a1 = __shfl(cnt1, from), b_0 = __shfl(cnt0, from + 1), b_1 = __shfl(cnt1, from + 1);
      const uint32_t va = lane < 32 ? a0 : a1, vb = lane < 32 ? b_0 : b_1;
      if (P.hits != nullptr)
      {
        uint16_t *dst = P.hits + blk * P.K;
        if (((uintptr_t)dst & 3u) == 0 && e0 + 1 < P.K)
        {
          *(uint32_t *)(dst + e0) = va | (vb << 16);
        }
        else
        {
          if (e0 < P.K)
          {
            dst[e0] = (uint16_t)va;
          }
          if (e0 + 1 < P.K)
          {
            dst[e0 + 1] = (uint16_t)vb;
          }
        }
      }
      uint32_t mine = 0;                                   // lane g keeps the key of group g
#pragma unroll
      for (uint32_t g = 0; g < kDcsGroups; g++)
      {
        // more hits win, then the lower index; 0 for a group without entries: best 255 - 0 = kDcsNoBest, 0 hits
        uint32_t key = max(grp0 == g ? (cnt0 << 8) | (255u - lane) : 0u, grp1 == g ? (cnt1 << 8) | (191u - lane) : 0u);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
        {
          key = max(key, (uint32_t)__shfl_xor((int)key, off));
        }
        mine = lane == g ? key : mine;
      }
      if (lane < kDcsGroups)
      {
        if (P.best != nullptr)
        {
          P.best[blk * kDcsGroups + lane] = (uint8_t)(255u - (mine & 255u));
        }
        if (P.present != nullptr)
        {
          P.present[blk * kDcsGroups + lane] = (mine >> 8) >= list->min_hits[lane] ? 1 : 0;
        }
      }
    }
    __syncthreads();

    // the state, or the bit array a tile down
    if (last)
    {
      if (tid < kDcsBitDw)
      {
        st_out[kDcsHistDw + tid] = bits[nb * (kDcsBlock / 32) + tid];
      }
    }
    else
    {
      const uint32_t keep = tid < kDcsBitDw ? bits[kDcsTileBitDw + tid] : 0u;
      __syncthreads();
      if (tid < kDcsBitDw)
      {
        bits[tid] = keep;
      }
    }
  }
}

} // namespace hrfd

// ------------------------------------------------------------------ host side
struct hrfd_dcs
{
  hrfd::BankCore core;
  uint32_t n_channels = 0;

  // host settings, under core.mu
  std::vector<int16_t> taps;
  uint32_t canon[hrfd::kDcsMaxCodes];      // in list order
  uint8_t group[hrfd::kDcsMaxCodes];
  uint32_t min_hits[hrfd::kDcsGroups];
  uint32_t K = 0;
  bool taps_dirty = true, list_dirty = true;
  hrfd::BankHistory hist;                  // rows of kDcsStateDw dwords

  // pinned staging: the packed taps, the list, the fresh flags
  hrfd::PinnedBuf<uint8_t> h_stage;
  size_t off_list = 0, off_fresh = 0;
  hrfd::DevBuf<uint2> d_taps;              // [kAudioMaxJ]
  hrfd::DevBuf<hrfd::DcsList> d_list;      // [1]

  // host-path staging
  hrfd::DevBuf<int16_t> d_pcm;
  hrfd::DevBuf<uint32_t> d_n_pcm;
  hrfd::DevBuf<uint16_t> d_hits;
  hrfd::DevBuf<uint8_t> d_best, d_present;
};

extern "C" int hrfd_dcs_create(uint32_t n_channels, int device, hrfd_dcs **out)
{
  using namespace hrfd;
  if (out != nullptr)
  {
    *out = nullptr;
  }
  BANK_TRY(dcs_check_create("hrfd_dcs_create", n_channels, out));
  hrfd_dcs *d = nullptr;
  BANK_TRY(bank_new("hrfd_dcs_create", device, &d));
  const size_t C = n_channels;
  d->n_channels = n_channels;
  d->taps.assign(1, (int16_t)16384);
  for (uint32_t g = 0; g < kDcsGroups; g++)
  {
    d->min_hits[g] = kDcsDefaultMinHits;
  }
  d->off_list = sizeof(uint2) * kAudioMaxJ;
  d->off_fresh = d->off_list + sizeof(DcsList);
  if (!(d->d_taps.alloc(kAudioMaxJ) && d->d_list.alloc(1) && d->hist.alloc(C, kDcsStateDw) && d->h_stage.alloc(d->off_fresh + C)))
  {
    (void)hipGetLastError();
    bank_free(d);
    return fail(HRFD_ENOMEM, "hrfd_dcs_create: device allocation failed");
  }
  *out = d;
  return HRFD_OK;
}

extern "C" int hrfd_dcs_destroy(hrfd_dcs *d)
{
  if (d != nullptr)
  {
    hrfd::bank_free(d);
  }
  return HRFD_OK;
}

// another filter makes the kept samples and slicer bits meaningless: every channel starts from zeros, as hrfd_audio_set_taps
extern "C" int hrfd_dcs_set_taps(hrfd_dcs *d, const int16_t *taps, uint32_t n)
{
  BANK_TRY(hrfd::dcs_check_taps("hrfd_dcs_set_taps", taps, n));
  BANK_TRY(hrfd::bank_need_handle("hrfd_dcs_set_taps", d));
  std::lock_guard<std::mutex> g(d->core.mu);
  d->taps.assign(taps, taps + n);
  d->taps_dirty = true;
  d->hist.mark(HRFD_ALL_CHANNELS);
  return HRFD_OK;
}

// the state stays: the slicer bits are facts about the signal, whatever list they are read against
extern "C" int hrfd_dcs_set_codes(hrfd_dcs *d, const uint16_t *codes, const uint8_t *inverted, const uint8_t *groups, uint32_t n)
{
  using namespace hrfd;
  BANK_TRY(dcs_check_codes("hrfd_dcs_set_codes", codes, inverted, groups, n));
  BANK_TRY(bank_need_handle("hrfd_dcs_set_codes", d));
  std::lock_guard<std::mutex> g(d->core.mu);
  for (uint32_t k = 0; k < n; k++)
  {
    d->canon[k] = dcs_canonical(dcs_word(codes[k], inverted != nullptr && inverted[k] != 0));
    d->group[k] = groups != nullptr ? groups[k] : 0;
  }
  d->K = n;
  d->list_dirty = true;
  return HRFD_OK;
}

extern "C" int hrfd_dcs_n_codes(hrfd_dcs *d, uint32_t *n)
{
  if (n == nullptr)
  {
    return fail(HRFD_EINVAL, "hrfd_dcs_n_codes: NULL result");
  }
  BANK_TRY(hrfd::bank_need_handle("hrfd_dcs_n_codes", d));
  std::lock_guard<std::mutex> g(d->core.mu);
  *n = d->K;
  return HRFD_OK;
}

extern "C" int hrfd_dcs_set_min_hits(hrfd_dcs *d, uint32_t group, uint32_t n)
{
  BANK_TRY(hrfd::dcs_check_min_hits("hrfd_dcs_set_min_hits", group, n));
  BANK_TRY(hrfd::bank_need_handle("hrfd_dcs_set_min_hits", d));
  std::lock_guard<std::mutex> g(d->core.mu);
  hrfd::bank_each_selected(hrfd::kDcsGroups, group, [&](uint32_t i) { d->min_hits[i] = n; });
  d->list_dirty = true;
  return HRFD_OK;
}

extern "C" int hrfd_dcs_reset(hrfd_dcs *d, uint32_t channel) { return hrfd::bank_reset_history(d, "hrfd_dcs_reset", channel); }

extern "C" int hrfd_dcs_code_word(uint32_t code, int inverted, uint32_t *word, uint32_t *canonical)
{
  if (code > 0777)
  {
    return fail(HRFD_EINVAL, "hrfd_dcs_code_word: code %u (three octal digits: 0..511)", code);
  }
  if (word == nullptr && canonical == nullptr)
  {
    return fail(HRFD_EINVAL, "hrfd_dcs_code_word: NULL result");
  }
  const uint32_t w = hrfd::dcs_word(code, inverted != 0);
  if (word != nullptr)
  {
    *word = w;
  }
  if (canonical != nullptr)
  {
    *canonical = hrfd::dcs_canonical(w);
  }
  return HRFD_OK;
}

static int dcs_check_process(hrfd_dcs *d, const char *who, const void *pcm, uint64_t stride, bool device_entry, const void *n_pcm,
                             uint32_t n_blocks, const void *hits, const void *best, const void *present)
{
  BANK_TRY(hrfd::dcs_check_call(who, pcm, stride, device_entry, n_pcm, n_blocks, hits, best, present));
  return hrfd::bank_need_handle(who, d);
}

// one call on `st`: what the setters changed, then k_dcs, one workgroup per channel.  staged_K: the list length the blocking
// host entry sized its hits by, or NULL: a set_codes from another thread since then ends the call before anything is touched
static int dcs_launch(hrfd_dcs *d, const int16_t *d_pcm, uint64_t stride, const uint32_t *d_n_pcm, uint32_t n_blocks, uint16_t *d_hits,
                      uint8_t *d_best, uint8_t *d_present, hipStream_t st, const uint32_t *staged_K = nullptr)
{
  using namespace hrfd;
  BANK_TRY(d->core.order_behind_last(st));
  DcsParams P;
  {
    std::lock_guard<std::mutex> g(d->core.mu);
    P.T = (uint32_t)d->taps.size();
    P.J = ((uint32_t)bank_packed_len((int)P.T) + kAudioStep - 1) / kAudioStep * kAudioStep;
    P.K = d->K;
    if (staged_K != nullptr && *staged_K != P.K)
    {
      return fail(HRFD_ESTATE, "hrfd_dcs_process: the code list changed from %u to %u entries while the call was staged", *staged_K, P.K);
    }
    P.reset = d->hist.reset();
    P.state_in = d->hist.in();
    P.state_out = d->hist.out();
    d->hist.flip();
    if (d->taps_dirty || d->list_dirty || d->hist.any_fresh)
    {
      BANK_TRY(d->core.staging_wait());
      if (d->taps_dirty)
      {
        bank_pack_taps(d->taps.data(), (int)P.T, (uint2 *)d->h_stage.p, (int)P.J);
        HIP_TRY(hipMemcpyAsync(d->d_taps, d->h_stage, sizeof(uint2) * P.J, hipMemcpyHostToDevice, st));
      }
      if (d->list_dirty)
      {
        DcsList *l = (DcsList *)(d->h_stage + d->off_list);
        dcs_sorted_list(d->canon, d->K, l->sorted, l->entry);
        memset(l->group, 0, sizeof(l->group));
        memcpy(l->group, d->group, d->K);
        memcpy(l->min_hits, d->min_hits, sizeof(l->min_hits));
        HIP_TRY(hipMemcpyAsync(d->d_list, l, sizeof(DcsList), hipMemcpyHostToDevice, st));
      }
      BANK_TRY(d->hist.upload(d->h_stage + d->off_fresh, st));
      d->taps_dirty = d->list_dirty = false;
      BANK_TRY(d->core.staging_sent(st));
    }
  }
  P.pcm = d_pcm;
  P.stride = stride;
  P.n_pcm = d_n_pcm;
  P.hits = d_hits;
  P.best = d_best;
  P.present = d_present;
  P.n_blocks = n_blocks;
  hipLaunchKernelGGL(k_dcs, dim3(d->n_channels), dim3(kDcsThreads), 0, st, P, (const uint2 *)d->d_taps.p, (const DcsList *)d->d_list.p);
  BANK_TRY(bank_launch_ok("k_dcs"));
  d->core.launched_on(st);
  return HRFD_OK;
}

extern "C" int hrfd_dcs_process_device(hrfd_dcs *d, const int16_t *d_pcm, uint64_t channel_stride_bytes, const uint32_t *d_n_pcm,
                                       uint32_t n_blocks, uint16_t *d_hits, uint8_t *d_best, uint8_t *d_present, void *stream)
{
  BANK_TRY(dcs_check_process(d, "hrfd_dcs_process_device", d_pcm, channel_stride_bytes, true, d_n_pcm, n_blocks, d_hits, d_best,
                             d_present));
  HIP_TRY(hipSetDevice(d->core.device));
  return dcs_launch(d, d_pcm, channel_stride_bytes, d_n_pcm, n_blocks, d_hits, d_best, d_present, d->core.stream_or_own(stream));
}

extern "C" int hrfd_dcs_process(hrfd_dcs *d, const int16_t *pcm, const uint32_t *n_pcm, uint32_t n_blocks, uint16_t *hits,
                                uint8_t *best, uint8_t *present)
{
  using namespace hrfd;
  BANK_TRY(dcs_check_process(d, "hrfd_dcs_process", pcm, 0, false, n_pcm, n_blocks, hits, best, present));
  BankHostCall call(d->core);
  uint32_t K;
  {
    std::lock_guard<std::mutex> g(d->core.mu);
    K = d->K;
  }
  const size_t C = d->n_channels, row = 2 * (size_t)kDcsBlock * n_blocks, V = C * n_blocks * kDcsGroups;
  const size_t H = 2 * C * n_blocks * K;                   // (an empty list leaves hits untouched)
  const int16_t *d_pcm = call.up(d->d_pcm, pcm, row * C);
  const uint32_t *d_n_pcm = call.up(d->d_n_pcm, n_pcm, 4 * C * n_blocks);
  uint16_t *d_hits = call.room(d->d_hits, hits, H > 0 ? H : 2);
  uint8_t *d_best = call.room(d->d_best, best, V), *d_present = call.room(d->d_present, present, V);
  BANK_TRY(call.rc);
  BANK_TRY(dcs_launch(d, d_pcm, row, d_n_pcm, n_blocks, d_hits, d_best, d_present, call.st, &K));
  call.down(H > 0 ? hits : nullptr, d_hits, H);
  call.down(best, d_best, V);
  call.down(present, d_present, V);
  return call.finish();
}

// the contract's loop over ONE channel, no device needed (include/hrfd_debug.h)
extern "C" int hrfd_dcs_debug_slow(const int16_t *taps, uint32_t n_taps, const uint16_t *codes, const uint8_t *inverted,
                                   const uint8_t *groups, uint32_t n_codes, const uint32_t *min_hits4, const int16_t *pcm,
                                   const uint32_t *n_pcm, uint32_t n_blocks, uint32_t *state300, uint16_t *hits, uint8_t *best,
                                   uint8_t *present)
{
  using namespace hrfd;
  const char *who = "hrfd_dcs_debug_slow";
  BANK_TRY(dcs_check_taps(who, taps, n_taps));
  BANK_TRY(dcs_check_codes(who, codes, inverted, groups, n_codes));
  if (min_hits4 == nullptr || state300 == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: NULL argument", who);
  }
  for (uint32_t g = 0; g < kDcsGroups; g++)
  {
    BANK_TRY(dcs_check_min_hits(who, g, min_hits4[g]));
  }
  BANK_TRY(dcs_check_call(who, pcm, 0, false, n_pcm, n_blocks, hits, best, present));
  uint32_t canon[kDcsMaxCodes];
  uint8_t group[kDcsMaxCodes];
  for (uint32_t k = 0; k < n_codes; k++)
  {
    canon[k] = dcs_canonical(dcs_word(codes[k], inverted != nullptr && inverted[k] != 0));
    group[k] = groups != nullptr ? groups[k] : 0;
  }
  dcs_channel_slow(pcm, n_pcm, n_blocks, taps, n_taps, canon, group, n_codes, min_hits4, state300, hits, best, present);
  return HRFD_OK;
}
