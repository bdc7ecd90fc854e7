// Sanitizer harness for the modulator launch's HIP-free part (hackrfdiags_amd/csrc/hrfd_tx_slices.h), CPU only: compiled
// as plain C++ under -fsanitize=address,undefined (tests/test_tx_slices_model.py).
//   san_tx_slices cuts    n_per_channel on stdin, one per line; prints the WBFM and the FM slices of each
//   san_tx_slices grids   "kind n_channels n_per_channel scan_kind" per line; prints tx_check_call's answer and, for an
//                         accepted call, the grid of every launch of the call, whole and sliced
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

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
#include "../../hackrfdiags_amd/csrc/hrfd_tx_slices.h"

using namespace hrfd;

static const char *const kScan[4] = {"rows8", "rows", "scan64", "plain"};

// guard words around the cuts: a slice too many lands on one of them
struct Cuts
{
  uint32_t before;
  uint32_t at[kTxMaxSlices];
  uint32_t after;
};

static int wbfm_cuts(uint32_t n, Cuts &c)
{
  c.before = c.after = 0xdeadbeefu;
  const int k = tx_wbfm_cuts(n, kTxMaxSlices, c.at);
  if (k < 1 || k > kTxMaxSlices || c.before != 0xdeadbeefu || c.after != 0xdeadbeefu)
  {
    printf("san_tx_slices: %d slices for n = %u\n", k, n);
    return -1;
  }
  return k;
}

static int run_cuts()
{
  unsigned long long v;
  while (scanf("%llu", &v) == 1)
  {
    const uint32_t n = (uint32_t)v;
    Cuts c;
    const int k = wbfm_cuts(n, c);
    if (k < 0) return 1;
    printf("%u wbfm %d %d", n, (int)tx_wbfm_sliceable(n), k);
    for (int i = 0; i < k; i++) printf(" %u", c.at[i]);
    printf(" fm %d", (int)tx_fm_sliceable(n));
    if (tx_fm_sliceable(n))
    {
      uint32_t f[4];
      tx_fm_cuts(n, f);
      printf(" %u %u %u %u", f[0], f[1], f[2], f[3]);
    }
    printf("\n");
  }
  return 0;
}

static void print_scan(int scan_kind, uint32_t C, uint64_t steps, uint64_t stride)
{
  const TxScan k = tx_scan_kernel(scan_kind, C, steps, stride);
  printf(" %s %u", kScan[k], tx_scan_grid(k, C));
}

static int run_grids()
{
  long long kind, scan_kind;
  unsigned long long vc, vn;
  while (scanf("%lld %llu %llu %lld", &kind, &vc, &vn, &scan_kind) == 4)
  {
    const uint32_t C = (uint32_t)vc, n = (uint32_t)vn;
    g_text[0] = 0;
    const int rc = tx_check_call("who", (int)kind, C, n);
    if (rc != HRFD_OK)
    {
      printf("%d %s\n", rc, g_text);
      continue;
    }
    printf("0 mod %u base %u", tx_mod_grid(C, n), tx_base_grid(C, n));
    if (kind == HRFD_MOD_WBFM)
    {
      printf(" tail %u rails %u", tx_wb_tail_grid(C, n, 512u), tx_wb_rails_grid(C, n, 512u));
      print_scan((int)scan_kind, C, (uint64_t)n * 32, (uint64_t)n * 32);
      Cuts c;
      const int k = wbfm_cuts(n, c);
      if (k < 0) return 1;
      for (int i = 0; i < k && k > 1; i++)
      {
        const uint32_t lo = i ? c.at[i - 1] : 0u, len = c.at[i] - lo;
        printf(" | %u %u %u", tx_mod_grid(C, len), tx_wb_tail_grid(C, len, 384u), tx_wb_rails_grid(C, len, 384u));
        print_scan((int)scan_kind, C, (uint64_t)len * 32, (uint64_t)n * 32);
      }
    }
    if (kind == HRFD_MOD_FM)
    {
      print_scan((int)scan_kind, C, n, n);
      uint32_t f[4];
      for (int i = 0; i < 3 && tx_fm_sliceable(n); i++)
      {
        tx_fm_cuts(n, f);
        const uint32_t len = f[i + 1] - f[i];
        printf(" | %u %u", tx_mod_grid(C, len), tx_base_grid(C, len));
        print_scan((int)scan_kind, C, len, n);
      }
    }
    printf("\n");
  }
  return 0;
}

int main(int argc, char **argv)
{
  const char *what = argc > 1 ? argv[1] : "";
  if (strcmp(what, "cuts") == 0) return run_cuts();
  if (strcmp(what, "grids") == 0) return run_grids();
  printf("usage: san_tx_slices cuts | grids\n");
  return 2;
}
