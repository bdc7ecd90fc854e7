// Sanitizer harness for the HIP-free part of the HDLC framer bank (hackrfdiags_amd/csrc/hrfd_hdlcgen.h), CPU only: compiled as
// plain C++ under -fsanitize=address,undefined (tests/test_hdlcgen_sanitizers.py).  Every check at its limit with its text;
// the rules on their boundaries (a lane's byte behind every run, the run operator against a walk, the check sequence as a
// sum against the register's loop for every length, the bound); and the slow loop with every buffer of exactly the size the
// contract gives it: a row of bits of exactly n_bits bytes, one byte short of a frame, rows of records cut at every multiple
// of 4, the longest frame of ones, and random rows of random bytes as records.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/hrfd.h"
static char g_err[512];
static int fail(int code, const char *fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
#include "../../hackrfdiags_amd/csrc/hrfd_hdlcgen.h"

using namespace hrfd;

#define CHECK(cond)                                                    \
  do                                                                   \
  {                                                                    \
    if (!(cond))                                                       \
    {                                                                  \
      printf("san_hdlcgen: line %d: %s (%s)\n", __LINE__, #cond, g_err); \
      return 1;                                                        \
    }                                                                  \
  } while (0)

// refused with HRFD_EINVAL, a text that starts with the function's name and holds `word`
static bool refused(int rc, const char *word)
{
  return rc == HRFD_EINVAL && strncmp(g_err, "who: ", 5) == 0 && strstr(g_err, word) != nullptr;
}

static int check_the_checks()
{
  static_assert(kHdlcgenMaxBits == HRFD_HDLCGEN_MAX_BITS && kHdlcgenMaxFlags == HRFD_HDLCGEN_MAX_FLAGS, "the header's limits are the public ones");
  static_assert(kHdlcgenMaxFrame == 9820 && kHdlcMaxPayload < (1u << kHdlcgenCrcLevels), "the longest frame, and the table's levels reach it");
  int out = 0;
  for (uint32_t c : {0u, 65537u, 0xffffffffu})
  {
    CHECK(refused(hdlcgen_check_create("who", c, &out), "channels"));
  }
  CHECK(refused(hdlcgen_check_create("who", 1, nullptr), "result pointer") && hdlcgen_check_create("who", 65536, &out) == HRFD_OK);
  CHECK(hdlcgen_check_flags("who", 0, 1, 1) == HRFD_OK && hdlcgen_check_flags("who", 255, 255, 255) == HRFD_OK);
  CHECK(refused(hdlcgen_check_flags("who", 256, 1, 1), "n_lead_flags 256") && refused(hdlcgen_check_flags("who", 0, 0, 1), "n_between 0"));
  CHECK(refused(hdlcgen_check_flags("who", 0, 256, 1), "n_between 256") && refused(hdlcgen_check_flags("who", 0, 1, 0), "n_tail_flags 0"));
  CHECK(refused(hdlcgen_check_flags("who", 0, 1, 256), "n_tail_flags 256"));
  for (uint32_t n : {0u, (1u << 20) + 1u, 0xffffffffu})
  {
    CHECK(refused(hdlcgen_check_max_bits("who", n), "max_bits"));
  }
  CHECK(hdlcgen_check_max_bits("who", 1) == HRFD_OK && hdlcgen_check_max_bits("who", 1u << 20) == HRFD_OK);

  const HdlcgenFlags def{12, 2, 3}, most{255, 255, 255};
  uint32_t v = 7;
  CHECK(refused(hdlcgen_check_bound("who", 1, 1, def, nullptr), "result pointer"));
  CHECK(refused(hdlcgen_check_bound("who", 0, 0, def, &v), "frames of") && refused(hdlcgen_check_bound("who", 2, 1, def, &v), "frames of"));
  CHECK(refused(hdlcgen_check_bound("who", 1, 1022, def, &v), "frames of") && refused(hdlcgen_check_bound("who", 1, 1ull << 63, def, &v), "frames of"));
  CHECK(refused(hdlcgen_check_bound("who", 0xffffffffu, 1ull << 40, def, &v), "more than one call") && v == 7);
  CHECK(hdlcgen_check_bound("who", 1, 2, def, &v) == HRFD_OK && v == 32 + 6 + 8 * 15);
  CHECK(hdlcgen_check_bound("who", 3, 30, most, &v) == HRFD_OK && v == 288 + 57 + 8 * 255 * 4);
  CHECK(hdlcgen_check_bound("who", 106, 106 * 1021, HdlcgenFlags{0, 1, 1}, &v) == HRFD_OK && v <= (1u << 20));
  CHECK(refused(hdlcgen_check_bound("who", 106, 106 * 1021, most, &v), "more than one call"));

  alignas(16) static char buf[8192];
  const void *r = buf, *f = buf + 1024, *b = buf + 2049, *n = buf + 4096, *s = buf + 4100, *d = buf + 4104;
  CHECK(hdlcgen_check_call("who", r, 68, 64, true, f, b, 101, 100, n, s, d, 1) == HRFD_OK);
  CHECK(hdlcgen_check_call("who", r, 0, 4, false, f, b, 0, 1u << 20, n, nullptr, nullptr, 1) == HRFD_OK);
  CHECK(refused(hdlcgen_check_call("who", r, 68, 64, true, f, b, 101, 0, n, s, d, 1), "max_bits"));
  for (uint32_t ib : {0u, 2u, 6u, 63u})
  {
    CHECK(refused(hdlcgen_check_call("who", r, 68, ib, true, f, b, 101, 100, n, s, d, 1), "in_bytes"));
  }
  CHECK(refused(hdlcgen_check_call("who", r, 60, 64, true, f, b, 101, 100, n, s, d, 1), "in_stride_bytes 60"));
  CHECK(refused(hdlcgen_check_call("who", r, 66, 64, true, f, b, 101, 100, n, s, d, 1), "in_stride_bytes 66"));
  CHECK(refused(hdlcgen_check_call("who", r, 68, 64, true, f, b, 99, 100, n, s, d, 1), "bits_stride_bytes 99"));
  CHECK(refused(hdlcgen_check_call("who", buf + 2, 68, 64, true, f, b, 101, 100, n, s, d, 1), "4-byte aligned address"));
  CHECK(refused(hdlcgen_check_call("who", r, 68, 64, true, buf + 1025, b, 101, 100, n, s, d, 1), "must be 4-byte aligned"));
  CHECK(refused(hdlcgen_check_call("who", r, 68, 64, true, f, b, 101, 100, buf + 4097, s, d, 1), "must be 4-byte aligned"));
  CHECK(refused(hdlcgen_check_call("who", r, 68, 64, true, f, b, 101, 100, n, buf + 4102, d, 1), "must be 4-byte aligned"));
  CHECK(refused(hdlcgen_check_call("who", r, 68, 64, true, f, b, 101, 100, n, s, buf + 4107, 1), "must be 4-byte aligned"));
  CHECK(refused(hdlcgen_check_call("who", nullptr, 68, 64, true, f, b, 101, 100, n, s, d, 1), "NULL argument"));
  CHECK(refused(hdlcgen_check_call("who", r, 68, 64, true, nullptr, b, 101, 100, n, s, d, 1), "NULL argument"));
  CHECK(refused(hdlcgen_check_call("who", r, 68, 64, true, f, nullptr, 101, 100, n, s, d, 1), "NULL argument"));
  CHECK(refused(hdlcgen_check_call("who", r, 68, 64, true, f, b, 101, 100, nullptr, s, d, 1), "NULL argument"));
  // the rows of bits on the records: from byte 64 on, one row of 20 lies behind channel 0's records and is all the check
  // knows of without a handle; three rows reach channel 1's, which begin at byte 68
  CHECK(hdlcgen_check_call("who", r, 68, 64, true, f, buf + 64, 20, 20, n, s, d, 1) == HRFD_OK);
  CHECK(refused(hdlcgen_check_call("who", r, 68, 64, true, f, buf + 64, 20, 20, n, s, d, 3), "overlaps"));
  CHECK(refused(hdlcgen_check_call("who", r, 68, 64, true, f, buf + 63, 20, 20, n, s, d, 1), "overlaps"));
  CHECK(hdlcgen_check_call("who", r, 68, 64, true, f, buf + 200, 20, 20, n, s, d, 3) == HRFD_OK);
  return 0;
}

// ---- the rules against walks
static uint32_t crc_of(const std::vector<uint8_t> &p)
{
  uint32_t crc = 0xFFFFu;
  for (uint8_t v : p)
  {
    crc = hdlc_crc_byte(crc, v);
  }
  return crc ^ 0xFFFFu;
}

static int check_the_rules()
{
  // a lane's byte behind every run: against a walk over the bits
  for (uint32_t b = 0; b < 256; b++)
  {
    uint32_t trail = 0;
    for (uint32_t i = 0; i < 8; i++)
    {
      trail = ((b >> i) & 1u) != 0 ? trail + 1 : 0;
    }
    CHECK(hdlcgen_run_of_byte(b) == (b == 255 ? (kHdlcgenRunAll | 8u) : trail));
    for (uint32_t run = 0; run < 23; run++)
    {
      uint32_t ones = run % 5, want = 0, n = 0;
      for (uint32_t i = 0; i < 8; i++)
      {
        const uint32_t bit = (b >> i) & 1u;
        want |= bit << n++;
        ones = bit ? ones + 1 : 0;
        if (ones == 5)
        {
          n++;
          ones = 0;
        }
      }
      uint32_t got = 0xdead;
      CHECK(hdlcgen_stuff_byte(b, run, &got) == n && got == want && n >= 8 && n <= 10);
    }
  }
  // the run operator: joined over random bytes in any grouping it is the run a walk finds
  uint32_t seed = 99;
  for (int round = 0; round < 200; round++)
  {
    std::vector<uint8_t> p(1 + (seed >> 9) % 40);
    for (uint8_t &v : p)
    {
      seed = seed * 1664525u + 1013904223u;
      v = (seed >> 29) != 0 ? 0xFF : (uint8_t)(seed >> 16);             // mostly 0xFF: runs over many bytes
    }
    uint32_t walk = 0, left = 0;                                     // left: the element 0, no run in front of the frame
    for (size_t i = 0; i < p.size(); i++)
    {
      CHECK((left & kHdlcgenRunAll) == 0 && left == walk);
      for (uint32_t k = 0; k < 8; k++)
      {
        walk = ((p[i] >> k) & 1u) != 0 ? walk + 1 : 0;
      }
      // the pair (i, i + 1) joined first, then with what lies in front: the operator is associative
      if (i + 1 < p.size())
      {
        const uint32_t pair = hdlcgen_run_join(hdlcgen_run_of_byte(p[i]), hdlcgen_run_of_byte(p[i + 1]));
        const uint32_t one = hdlcgen_run_join(hdlcgen_run_join(left, hdlcgen_run_of_byte(p[i])), hdlcgen_run_of_byte(p[i + 1]));
        CHECK(hdlcgen_run_join(left, pair) == one);
      }
      left = hdlcgen_run_join(left, hdlcgen_run_of_byte(p[i]));
      CHECK(hdlcgen_run_join(kHdlcgenRunId, hdlcgen_run_of_byte(p[i])) == hdlcgen_run_of_byte(p[i]));
      CHECK(hdlcgen_run_join(left, kHdlcgenRunId) == left);
    }
  }
  // the check sequence as a sum, for every length
  static constexpr HdlcgenCrcPow pow = hdlcgen_crc_pow();
  CHECK(pow.pow[0][0] == hdlcgen_crc_m(1) && hdlcgen_crc_m(0) == 0);
  std::vector<uint8_t> p;
  for (uint32_t n = 1; n <= kHdlcMaxPayload; n++)
  {
    seed = seed * 1664525u + 1013904223u;
    p.push_back((uint8_t)(seed >> 24));
    if (n > 70 && n % 97 != 0 && n < 1019)
    {
      continue;
    }
    uint32_t sum = 0;
    for (uint32_t i = 0; i < n; i++)
    {
      sum ^= hdlcgen_crc_term(pow, p[i], i, n);
    }
    CHECK((~sum & 0xFFFFu) == crc_of(p));
  }
  CHECK(crc_of({'1', '2', '3', '4', '5', '6', '7', '8', '9'}) == 0x906E && crc_of({0xFF, 0xFF}) == 0xFFFF);
  CHECK(hdlcgen_bound(1, 2, HdlcgenFlags{0, 1, 1}) == 46 && hdlcgen_bound(106, 106 * 1021, HdlcgenFlags{255, 255, 255}) > (1u << 20));
  return 0;
}

// ---- rows
static void put_record(std::vector<uint8_t> &row, const std::vector<uint8_t> &payload, uint32_t n_field)
{
  const uint8_t head[8] = {0xEE, 0xEE, 0xEE, 0xEE, (uint8_t)(n_field & 255), (uint8_t)(n_field >> 8), 0xCC, 0xCC};     // end_bit and fcs: ignored
  row.insert(row.end(), head, head + 8);
  row.insert(row.end(), payload.begin(), payload.end());
  row.resize((row.size() + 3) & ~(size_t)3, 0);
}

struct Result
{
  std::vector<uint8_t> bits;                   // exactly max_bits: the sanitizer sees a byte too many
  uint32_t counts[3];
};

static Result run(const std::vector<uint8_t> &row, uint32_t in_bytes, uint32_t n_frames, const HdlcgenFlags &fl, uint32_t max_bits)
{
  Result r;
  r.bits.assign(max_bits, 0xA5);
  std::vector<uint8_t> copy(row.begin(), row.begin() + in_bytes);      // exactly the call's bytes
  hdlcgen_row_slow(copy.data(), in_bytes, n_frames, fl, r.bits.data(), max_bits, r.counts);
  return r;
}

// the frames of a row of bits by the receive side's rules (hrfd_hdlc.h), payloads only.  open: the row has no flag in front
// (lead = 0), so one is put there for the receive side, which opens a frame at a flag only
static std::vector<std::vector<uint8_t>> deframe(const uint8_t *bits, uint32_t n, bool open)
{
  std::vector<uint8_t> row;
  for (uint32_t i = 0; open && i < 8; i++)
  {
    row.push_back((uint8_t)((kHdlcgenFlag >> i) & 1u));
  }
  row.insert(row.end(), bits, bits + n);
  n = (uint32_t)row.size();
  HdlcState *st = new HdlcState();
  std::vector<uint8_t> out(hdlc_max_out(n > 0 ? n : 1, 1, kHdlcMaxPayload));
  uint32_t counts[3];
  hdlc_channel_slow(row.data(), n, HdlcLimits{1, kHdlcMaxPayload, 0}, st, out.data(), (uint32_t)out.size(), counts);
  delete st;
  std::vector<std::vector<uint8_t>> frames;
  size_t at = 0;
  for (uint32_t i = 0; i < counts[0]; i++)
  {
    hrfd_hdlc_record rec;
    memcpy(&rec, out.data() + at, sizeof(rec));
    frames.emplace_back(out.begin() + at + 8, out.begin() + at + 8 + rec.n_payload);
    at += hdlc_record_bytes(rec.n_payload);
  }
  if (counts[1] != 0 || counts[2] != 0)
  {
    frames.clear();
  }
  return frames;
}

static int check_the_rows()
{
  const std::vector<std::vector<uint8_t>> batch = {std::vector<uint8_t>(9, 0xFF), {'h', 'e', 'l', 'l', 'o'}, {0x00, 0xF8, 0x1F},
                                                   std::vector<uint8_t>(kHdlcMaxPayload, 0xFF), {0x7E}};
  std::vector<uint8_t> row;
  std::vector<uint32_t> ends;                  // the row's length behind every record
  for (const auto &p : batch)
  {
    put_record(row, p, (uint32_t)p.size());
    ends.push_back((uint32_t)row.size());
  }
  for (const HdlcgenFlags &fl : {HdlcgenFlags{12, 2, 3}, HdlcgenFlags{0, 1, 1}, HdlcgenFlags{255, 255, 255}})
  {
    uint64_t payload_bytes = 0;
    for (uint32_t k = 1; k <= batch.size(); k++)
    {
      payload_bytes += batch[k - 1].size();
      const uint32_t room = (uint32_t)hdlcgen_bound(k, payload_bytes, fl);
      Result all = run(row, (uint32_t)row.size(), k, fl, room);
      const uint32_t exact = all.counts[0];
      CHECK(all.counts[1] == k && all.counts[2] == 0 && exact <= room && (exact == room || all.bits[exact] == 0xA5));
      const auto frames = deframe(all.bits.data(), exact, fl.lead == 0);
      CHECK(frames.size() == k);
      for (uint32_t i = 0; i < k; i++)
      {
        CHECK(frames[i] == batch[i]);
      }
      // a row of exactly the length, one short of it, and the same frames from a row of records cut behind the k-th
      Result tight = run(row, (uint32_t)row.size(), (uint32_t)batch.size(), fl, exact);
      CHECK(tight.counts[0] == exact && tight.counts[1] == k && tight.counts[2] == batch.size() - k && memcmp(tight.bits.data(), all.bits.data(), exact) == 0);
      Result shorter = run(row, (uint32_t)row.size(), (uint32_t)batch.size(), fl, exact - 1);
      CHECK(shorter.counts[1] == k - 1 && shorter.counts[2] == batch.size() - k + 1 && shorter.counts[0] < exact);
      CHECK(k > 1 ? shorter.counts[0] > 0 : (shorter.counts[0] == 0 && shorter.bits[0] == 0xA5));
      Result cut = run(row, ends[k - 1], (uint32_t)batch.size(), fl, room);
      CHECK(cut.counts[0] == exact && cut.counts[1] == k && memcmp(cut.bits.data(), all.bits.data(), exact) == 0);
    }
  }
  // a row of records cut at every multiple of 4: the records that lie whole in it are framed
  const HdlcgenFlags def{12, 2, 3};
  for (uint32_t in_bytes = 4; in_bytes <= row.size(); in_bytes += 4)
  {
    uint32_t whole = 0;
    while (whole < ends.size() && ends[whole] <= in_bytes)
    {
      whole++;
    }
    Result r = run(row, in_bytes, 7, def, 1u << 15);
    CHECK(r.counts[1] == whole && r.counts[2] == 7 - whole);
  }
  // malformed lengths in the middle
  for (uint32_t n_field : {0u, 1022u, 0xFFFFu})
  {
    std::vector<uint8_t> bad;
    put_record(bad, batch[1], (uint32_t)batch[1].size());
    put_record(bad, batch[2], n_field);
    put_record(bad, batch[4], 1);
    Result r = run(bad, (uint32_t)bad.size(), 3, def, 4096);
    CHECK(r.counts[1] == 1 && r.counts[2] == 2 && deframe(r.bits.data(), r.counts[0], false).size() == 1);
  }
  // the stuffed zero behind a fifth one that is the frame's last bit: a check sequence whose last five bits are ones
  uint32_t seed = 5;
  for (int tries = 0, found = 0; found < 3; tries++)
  {
    CHECK(tries < 1000000);
    seed = seed * 1664525u + 1013904223u;
    const std::vector<uint8_t> p = {(uint8_t)(seed >> 8), (uint8_t)(seed >> 16), (uint8_t)(seed >> 24)};
    const uint32_t crc = crc_of(p);
    if ((crc >> 10) != 0x1F * 2u)              // bits 15..11 ones, bit 10 zero: a run of exactly five ends the frame
    {
      continue;
    }
    found++;
    std::vector<uint8_t> one;
    put_record(one, p, 3);
    Result r = run(one, (uint32_t)one.size(), 1, HdlcgenFlags{0, 1, 1}, 60);
    const uint32_t n = r.counts[0];
    CHECK(r.counts[1] == 1 && n >= 14 && r.bits[n - 9] == 0 && r.bits[n - 10] == 1 && r.bits[n - 14] == 1 && r.bits[n - 15] == 0);
    const auto frames = deframe(r.bits.data(), n, true);
    CHECK(frames.size() == 1 && frames[0] == p);
  }
  return 0;
}

static int check_random_rows()
{
  uint32_t seed = 4242;
  for (int round = 0; round < 300; round++)
  {
    std::vector<uint8_t> row(4 * (1 + (seed >> 7) % 300));
    for (uint8_t &v : row)
    {
      seed = seed * 1664525u + 1013904223u;
      v = (uint8_t)(seed >> 24);
    }
    for (size_t at = 5; at < row.size(); at += 8)
    {
      row[at] &= 1;                              // lengths that are often valid: the walk gets somewhere
    }
    seed = seed * 1664525u + 1013904223u;
    const uint32_t max_bits = 1 + (seed >> 8) % 20000, n_frames = (seed >> 3) % 9;
    const HdlcgenFlags fl{(seed >> 4) % 256, 1 + (seed >> 12) % 255, 1 + (seed >> 20) % 255};
    Result r = run(row, (uint32_t)row.size(), n_frames, fl, max_bits);
    CHECK(r.counts[0] <= max_bits && r.counts[1] + r.counts[2] == n_frames && (r.counts[1] == 0) == (r.counts[0] == 0));
    CHECK(deframe(r.bits.data(), r.counts[0], fl.lead == 0).size() == r.counts[1]);
  }
  return 0;
}

int main()
{
  if (check_the_checks() || check_the_rules() || check_the_rows() || check_random_rows())
  {
    return 1;
  }
  printf("san_hdlcgen ok\n");
  return 0;
}
