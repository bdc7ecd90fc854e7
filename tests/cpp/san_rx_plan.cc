// Sanitizer harness for the receive launch's HIP-free part (hackrfdiags_amd/csrc/hrfd_rx_plan.h), CPU only: compiled as
// plain C++ under -fsanitize=address,undefined (tests/test_sanitizers.py, tests/test_rx_plan_model.py).
//   san_rx_plan plan    cases on stdin, one per line; prints "case" and one line per step of rx_plan
//   san_rx_plan geom    calls of rx_geometry on stdin; prints its code, its text and its results
//   san_rx_plan lists   rx_build_lists and rx_max_threshold against brute force, random modes and subsets
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../../include/hrfd.h"
static char g_text[512];
static int fail(int code, const char *fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_text, sizeof(g_text), fmt, ap);
  va_end(ap);
  return code;
}
#include "../../hackrfdiags_amd/csrc/hrfd_rx_plan.h"

using namespace hrfd;

#define CHECK(cond)                                                \
  do                                                               \
  {                                                                \
    if (!(cond))                                                   \
    {                                                              \
      printf("san_rx_plan: line %d: %s\n", __LINE__, #cond);       \
      return 1;                                                    \
    }                                                              \
  } while (0)

static const char *const kNames[kRxKernels] = {
    "flow_bank", "flow_bank_dump", "flow_as", "flow_as_dump", "flow_fm", "flow_fm_dump", "flow_wb", "flow_wb_dump",
    "gated_wb", "gated_fm", "gated_as", "fir_as", "fir_as_256", "post_as", "fir_fm", "fir_fm_256", "fir_fm_arith",
    "blocks_none", "blocks_wb", "blocks_wb_256", "blocks_wb_arith", "finish"};

// a case: n_none n_am n_fm n_wb n_lsb n_usb | n_blocks n256 gain_db max_threshold warm_tiles | serial src256 subset dump |
// use_stream atan_mode fir_flow gated_pass run_len | tab_ok quad_ok arith_ok | has_dbg dbg_cap
// The channels are laid out mode by mode and go through rx_build_lists (as the whole bank, or as a subset of twice as
// many channels) for the counts.
static int run_plans()
{
  long long v[25];
  char line[512];
  long n_case = 0;
  while (fgets(line, sizeof(line), stdin) != nullptr)
  {
    int got = 0, pos = 0, adv = 0;
    while (got < 25 && sscanf(line + pos, "%lld%n", &v[got], &adv) == 1)
    {
      pos += adv;
      got++;
    }
    CHECK(got == 25);
    const bool subset = v[13] != 0;
    std::vector<ChanCfg> cfg;
    std::vector<uint32_t> members;
    for (int m = 0; m < 6; m++)
    {
      for (long long i = 0; i < v[m]; i++)
      {
        ChanCfg c;
        memset(&c, 0, sizeof(c));
        c.mode = m;
        if (subset)
        {
          cfg.push_back(c);                                // a channel of the same mode that is not in the subset
        }
        members.push_back((uint32_t)cfg.size());
        cfg.push_back(c);
      }
    }
    const uint32_t n = (uint32_t)cfg.size();
    std::vector<uint32_t> lists((size_t)kRxLists * n + 1);
    RxPlanIn in;
    rx_build_lists(cfg.data(), n, subset, members.data(), (uint32_t)members.size(), lists.data(), in.count);
    in.n_channels = n;
    in.n_blocks = (uint32_t)v[6];
    in.n256 = (uint32_t)v[7];
    in.gain_db = (uint32_t)v[8];
    in.max_threshold = (int32_t)v[9];
    in.warm_tiles = (int)v[10];
    in.serial = v[11] != 0;
    in.src256 = v[12] != 0;
    in.subset = subset;
    in.dump = v[14] != 0;
    in.use_stream = (int)v[15];
    in.atan_mode = (int)v[16];
    in.fir_flow = (int)v[17];
    in.gated_pass = (int)v[18];
    in.run_len = (int)v[19];
    in.tab_ok = v[20] != 0;
    in.quad_ok = v[21] != 0;
    in.arith_ok = v[22] != 0;
    in.has_dbg = v[23] != 0;
    in.dbg_cap = (size_t)v[24];
    const RxPlan plan = rx_plan(in);
    CHECK(plan.n >= 0 && plan.n < kRxMaxSteps);
    printf("case %ld %d\n", n_case++, plan.n);
    for (int i = 0; i < plan.n; i++)
    {
      const RxStep &s = plan.step[i];
      CHECK(s.kernel < kRxKernels);
      printf("%s %d %u %u %u %u %u %d %d %d %d\n", kNames[s.kernel], (int)s.list, s.n_list, s.grid, s.block, s.run_len, s.n_runs,
             s.warm_tiles, (int)s.self_finish, (int)s.dbg, (int)s.expire_once);
    }
  }
  return 0;
}

// a call: block_bytes n_blocks channel_stride out_b0 out_blocks serial src256 offgrid warm
static int run_geometry()
{
  unsigned long long v[9];
  while (scanf("%llu %llu %llu %llu %llu %llu %llu %llu %llu", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7], &v[8]) == 9)
  {
    RxGeometry g;
    memset(&g, 0, sizeof(g));
    g_text[0] = 0;
    const int rc = rx_geometry((uint32_t)v[0], (uint32_t)v[1], v[2], (uint32_t)v[3], (uint32_t)v[4], (int)v[5], (int)v[6], v[7] != 0,
                               (int)v[8], &g);
    if (rc != HRFD_OK)
    {
      printf("%d %s\n", rc, g_text);
    }
    else
    {
      printf("0 %d %u %d %d %d %d %d\n", (int)g.ragged, g.n256, g.warm_tiles, g.seed_terms, g.ntiles, g.origin, g.hal);
    }
  }
  return 0;
}

static int run_lists()
{
  std::mt19937 rng(11);
  for (int trial = 0; trial < 400; trial++)
  {
    const uint32_t n = 1 + rng() % 70;
    std::vector<ChanCfg> cfg(n);
    memset(cfg.data(), 0, sizeof(ChanCfg) * n);
    for (ChanCfg &c : cfg)
    {
      c.mode = trial % 5 == 0 ? (int)(trial / 5 % 6) : (int)(rng() % 6);           // one mode only, or any
      c.threshold = (int32_t)(rng() % 400) - 300;
    }
    // the whole bank (no subset), then subsets: empty, single, the whole bank as a subset, random
    for (int kind = 0; kind < 5; kind++)
    {
      std::vector<uint32_t> sub;
      for (uint32_t c = 0; c < n; c++)
      {
        if (kind == 3 || (kind == 4 && rng() % 3 == 0) || (kind == 2 && c == trial % n))
        {
          sub.push_back(c);
        }
      }
      const bool whole = kind == 0;
      std::vector<uint32_t> lists((size_t)kRxLists * n, 0xdeadbeefu);
      uint32_t counts[kRxLists];
      rx_build_lists(cfg.data(), n, !whole, sub.data(), (uint32_t)sub.size(), lists.data(), counts);
      for (int l = 0; l < kRxLists; l++)
      {
        // brute force: the members of list l, in channel order
        std::vector<uint32_t> want;
        for (uint32_t c = 0; c < n; c++)
        {
          const int m = cfg[c].mode;
          if (!whole && std::find(sub.begin(), sub.end(), c) == sub.end())
          {
            continue;
          }
          bool in;
          switch (l)
          {
            case 6: in = whole ? m != HRFD_MODE_WBFM : true; break;
            case 7: in = m == HRFD_MODE_AM || m == HRFD_MODE_LSB || m == HRFD_MODE_USB; break;
            case 8: in = false; break;
            case 9: in = whole && m != HRFD_MODE_NONE; break;
            default: in = m == l; break;
          }
          if (in) want.push_back(c);
        }
        CHECK(counts[l] == want.size());
        CHECK(std::equal(want.begin(), want.end(), lists.begin() + (size_t)l * n));
        for (uint32_t i = counts[l]; i < n; i++)
        {
          CHECK(lists[(size_t)l * n + i] == 0xdeadbeefu);    // nothing written behind a list
        }
      }
    }
    int32_t want_thr = INT32_MIN;
    for (const ChanCfg &c : cfg)
    {
      if (c.mode != HRFD_MODE_NONE) want_thr = std::max(want_thr, c.threshold);
    }
    CHECK(rx_max_threshold(cfg.data(), n) == want_thr);
  }
  printf("san_rx_plan lists ok\n");
  return 0;
}

int main(int argc, char **argv)
{
  const char *what = argc > 1 ? argv[1] : "";
  if (strcmp(what, "plan") == 0) return run_plans();
  if (strcmp(what, "geom") == 0) return run_geometry();
  if (strcmp(what, "lists") == 0) return run_lists();
  printf("usage: san_rx_plan plan | geom | lists\n");
  return 2;
}
