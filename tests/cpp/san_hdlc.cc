// Sanitizer harness for the HIP-free part of the HDLC bank (hackrfdiags_amd/csrc/hrfd_hdlc.h), CPU only: compiled as plain
// C++ under -fsanitize=address,undefined (tests/test_hdlc_sanitizers.py).  Every check at its limit with its text, the rules
// on their boundaries (the classes of a bit for every run, the CRC's residue, the record's size, the row bound at the limits),
// and the slow loop with every buffer of exactly the size the contract gives it: a frame of exactly cap bits and one of a bit
// more at P = 1, 5 and 1021, back-to-back minimal frames into a row of exactly max_out bytes and into one a record short, a
// stream cut at every bit against one call, and random bytes.
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
#include "../../hackrfdiags_amd/csrc/hrfd_hdlc.h"

using namespace hrfd;

#define CHECK(cond)                                                 \
  do                                                                \
  {                                                                 \
    if (!(cond))                                                    \
    {                                                               \
      printf("san_hdlc: line %d: %s (%s)\n", __LINE__, #cond, g_err); \
      return 1;                                                     \
    }                                                               \
  } while (0)

// refused with HRFD_EINVAL, a text that starts with the function's name and holds `word`
static bool refused(int rc, const char *word)
{
  return rc == HRFD_EINVAL && strncmp(g_err, "who: ", 5) == 0 && strstr(g_err, word) != nullptr;
}

static int check_the_checks()
{
  static_assert(kHdlcMaxBits == HRFD_HDLC_MAX_BITS && kHdlcMaxPayload == HRFD_HDLC_MAX_PAYLOAD, "the header's limits are the public ones");
  static_assert(sizeof(HdlcState) == 1040 && sizeof(hrfd_hdlc_record) == kHdlcHeader, "260 dwords of state, 8 bytes of header");
  static_assert(kHdlcBitValue == HRFD_AFSK_BIT && kHdlcBitCarrier == HRFD_AFSK_CARRIER, "the AFSK bank's byte");
  int out = 0;
  for (uint32_t c : {0u, 65537u, 0xffffffffu})
  {
    CHECK(refused(hdlc_check_create("who", c, &out), "channels"));
  }
  CHECK(refused(hdlc_check_create("who", 1, nullptr), "result pointer") && hdlc_check_create("who", 65536, &out) == HRFD_OK);

  for (uint32_t P : {0u, 1022u, 0xffffffffu})
  {
    CHECK(refused(hdlc_check_limits("who", 1, P), "max_payload"));
  }
  CHECK(refused(hdlc_check_limits("who", 0, 512), "min_payload 0") && refused(hdlc_check_limits("who", 513, 512), "min_payload 513"));
  CHECK(hdlc_check_limits("who", 1, 1) == HRFD_OK && hdlc_check_limits("who", 1021, 1021) == HRFD_OK && hdlc_check_limits("who", 1, 1021) == HRFD_OK);
  for (uint32_t n : {0u, (1u << 20) + 1u, 0xffffffffu})
  {
    CHECK(refused(hdlc_check_max_bits("who", n), "max_bits"));
  }
  CHECK(hdlc_check_max_bits("who", 1) == HRFD_OK && hdlc_check_max_bits("who", 1u << 20) == HRFD_OK);

  alignas(16) static char buf[4096];
  const void *b = buf + 1, *n = buf + 1024, *o = buf + 2048, *f = buf + 3072, *d = buf + 3076, *x = buf + 3080;
  CHECK(hdlc_check_call("who", b, 100, true, n, 100, o, 64, 64, f, x, d) == HRFD_OK);
  CHECK(hdlc_check_call("who", b, 0, false, n, 1u << 20, o, 0, 4, f, nullptr, d) == HRFD_OK);
  CHECK(refused(hdlc_check_call("who", b, 100, true, n, 0, o, 64, 64, f, x, d), "max_bits"));
  CHECK(refused(hdlc_check_call("who", b, 99, true, n, 100, o, 64, 64, f, x, d), "bits_stride_bytes 99"));
  for (uint32_t ob : {0u, 2u, 6u, 63u})
  {
    CHECK(refused(hdlc_check_call("who", b, 100, true, n, 100, o, 64, ob, f, x, d), "out_bytes"));
  }
  CHECK(refused(hdlc_check_call("who", b, 100, true, n, 100, o, 60, 64, f, x, d), "out_stride_bytes 60"));
  CHECK(refused(hdlc_check_call("who", b, 100, true, n, 100, o, 66, 64, f, x, d), "out_stride_bytes 66"));
  CHECK(refused(hdlc_check_call("who", b, 100, true, n, 100, buf + 2050, 64, 64, f, x, d), "4-byte aligned address"));
  CHECK(refused(hdlc_check_call("who", b, 100, true, buf + 1025, 100, o, 64, 64, f, x, d), "must be 4-byte aligned"));
  CHECK(refused(hdlc_check_call("who", b, 100, true, n, 100, o, 64, 64, buf + 3073, x, d), "must be 4-byte aligned"));
  CHECK(refused(hdlc_check_call("who", b, 100, true, n, 100, o, 64, 64, f, buf + 3082, d), "must be 4-byte aligned"));
  CHECK(refused(hdlc_check_call("who", b, 100, true, n, 100, o, 64, 64, f, x, buf + 3079), "must be 4-byte aligned"));
  CHECK(refused(hdlc_check_call("who", nullptr, 100, true, n, 100, o, 64, 64, f, x, d), "NULL argument"));
  CHECK(refused(hdlc_check_call("who", b, 100, true, nullptr, 100, o, 64, 64, f, x, d), "NULL argument"));
  CHECK(refused(hdlc_check_call("who", b, 100, true, n, 100, nullptr, 64, 64, f, x, d), "NULL argument"));
  CHECK(refused(hdlc_check_call("who", b, 100, true, n, 100, o, 64, 64, nullptr, x, d), "NULL argument"));
  CHECK(refused(hdlc_check_call("who", b, 100, true, n, 100, o, 64, 64, f, x, nullptr), "NULL argument"));
  return 0;
}

static int check_the_rules()
{
  for (uint32_t ones = 0; ones <= 7; ones++)
  {
    CHECK(hdlc_classify(1, ones) == (uint32_t)(kHdlcKeep | (ones >= 6 ? kHdlcAbort : 0)));
    CHECK(hdlc_classify(0, ones) == (uint32_t)(ones == 6 ? kHdlcFlag : (ones == 5 ? 0 : kHdlcKeep)));
    CHECK(hdlc_next_ones(1, ones) == (ones < 7 ? ones + 1 : 7) && hdlc_next_ones(0, ones) == 0);
  }
  // "123456789": CRC-16/X.25 is 0x906E; with it behind the data the register ends at the residue
  uint32_t crc = 0xFFFF;
  for (const char *p = "123456789"; *p; p++)
  {
    crc = hdlc_crc_byte(crc, (uint8_t)*p);
  }
  CHECK((crc ^ 0xFFFF) == 0x906E);
  crc = hdlc_crc_byte(hdlc_crc_byte(crc, 0x6E), 0x90);
  CHECK(crc == kHdlcResidue);
  CHECK(hdlc_record_bytes(0) == 8 && hdlc_record_bytes(1) == 12 && hdlc_record_bytes(4) == 12 && hdlc_record_bytes(1021) == 1032);
  CHECK(hdlc_cap(1) == 31 && hdlc_least(1) == 31 && hdlc_cap(1021) == 8191 && hdlc_cap(1021) <= 32 * kHdlcBitWords);
  CHECK(hdlc_max_out(1, 1, 512) == 524 && hdlc_max_out(32, 1, 1) == 12 && hdlc_max_out(33, 1, 1) == 24);
  CHECK(hdlc_max_out(1u << 20, 1, 1021) == ((11u * 32768u + 1021u + 131072u + 3u) & ~3u));
  const uint32_t words[3] = {0x89abcdefu, 0x01234567u, 0xffffffffu};
  CHECK(hdlc_byte_at(words, 0) == 0xef && hdlc_byte_at(words, 24) == 0x89 && hdlc_byte_at(words, 28) == 0x78 && hdlc_byte_at(words, 31) == 0xcf);
  return 0;
}

// ---- streams
static void put_flag(std::vector<uint8_t> &s)
{
  for (int b : {0, 1, 1, 1, 1, 1, 1, 0})
  {
    s.push_back((uint8_t)(b | 2));
  }
}

static void put_frame(std::vector<uint8_t> &s, const std::vector<uint8_t> &payload)
{
  uint32_t crc = 0xFFFF;
  for (uint8_t v : payload)
  {
    crc = hdlc_crc_byte(crc, v);
  }
  crc ^= 0xFFFF;
  std::vector<uint8_t> bytes = payload;
  bytes.push_back((uint8_t)(crc & 255));
  bytes.push_back((uint8_t)(crc >> 8));
  int ones = 0;
  for (uint8_t v : bytes)
  {
    for (int k = 0; k < 8; k++)
    {
      const int b = (v >> k) & 1;
      s.push_back((uint8_t)(b | 2));
      ones = b ? ones + 1 : 0;
      if (ones == 5)
      {
        s.push_back(2);
        ones = 0;
      }
    }
  }
}

struct Result
{
  std::vector<uint8_t> out;                    // exactly out_bytes: the sanitizer sees a byte too many
  uint32_t counts[3];
};

static Result run(const std::vector<uint8_t> &s, size_t from, size_t to, const HdlcLimits &lim, HdlcState *st, uint32_t out_bytes)
{
  Result r;
  r.out.assign(out_bytes, 0xA5);
  std::vector<uint8_t> row(s.begin() + from, s.begin() + to);        // a copy of exactly the call's bits
  hdlc_channel_slow(row.data(), (uint32_t)row.size(), lim, st, r.out.data(), out_bytes, r.counts);
  return r;
}

static int check_the_cap()
{
  for (uint32_t P : {1u, 5u, 1021u})
  {
    const HdlcLimits lim{1, P, 0};
    std::vector<uint8_t> s;
    put_flag(s);
    put_frame(s, std::vector<uint8_t>(P, 0x11));           // n reaches cap exactly at the closing flag
    put_flag(s);
    put_frame(s, std::vector<uint8_t>(P + 1, 0x11));       // a byte more: dead at n == cap
    put_flag(s);
    put_frame(s, std::vector<uint8_t>(1, 0x42));
    put_flag(s);
    HdlcState *st = new HdlcState();                       // on the heap: its end is guarded
    const uint32_t ob = hdlc_max_out((uint32_t)s.size(), 1, P);
    Result r = run(s, 0, s.size(), lim, st, ob);
    CHECK(r.counts[0] == 2 && r.counts[1] == 0 && r.counts[2] == 0);
    hrfd_hdlc_record rec;
    memcpy(&rec, r.out.data(), sizeof(rec));
    CHECK(rec.n_payload == P && r.out[8] == 0x11 && r.out[8 + P - 1] == 0x11);
    memcpy(&rec, r.out.data() + hdlc_record_bytes(P), sizeof(rec));
    CHECK(rec.n_payload == 1 && r.out[hdlc_record_bytes(P) + 8] == 0x42 && rec.end_bit == s.size() - 1);
    CHECK(r.out[hdlc_record_bytes(P) + 12] == 0xA5 && st->in_frame == 1 && st->n == 0 && st->ones == 0);
    // a stream that ends inside the over-long frame: the state holds at most cap bits
    *st = HdlcState();
    r = run(s, 0, s.size() - 40, lim, st, ob);
    CHECK(r.counts[0] == 1 && st->n <= hdlc_cap(P));
    delete st;
  }
  return 0;
}

static int check_the_row_bound_and_the_cuts()
{
  for (uint32_t m : {1u, 2u, 5u})
  {
    const HdlcLimits lim{m, 512, 0};
    std::vector<uint8_t> s;
    put_flag(s);
    for (int i = 0; i < 50; i++)
    {
      put_frame(s, std::vector<uint8_t>(m, (uint8_t)(2 * i + 2)));
      put_flag(s);
    }
    HdlcState st = HdlcState();
    const uint32_t ob = hdlc_max_out((uint32_t)s.size(), m, 512), size = hdlc_record_bytes(m);
    Result whole = run(s, 0, s.size(), lim, &st, ob);
    CHECK(whole.counts[0] == 50 && whole.counts[2] == 0 && ob >= 50 * size);
    st = HdlcState();
    Result tight = run(s, 0, s.size(), lim, &st, 50 * size);           // exactly the records
    CHECK(tight.counts[0] == 50 && tight.counts[2] == 0 && memcmp(tight.out.data(), whole.out.data(), 50 * size) == 0);
    st = HdlcState();
    Result less = run(s, 0, s.size(), lim, &st, 49 * size);
    CHECK(less.counts[0] == 49 && less.counts[2] == 1 && memcmp(less.out.data(), whole.out.data(), 49 * size) == 0);
    st = HdlcState();
    Result least = run(s, 0, s.size(), lim, &st, 4);
    CHECK(least.counts[0] == 0 && least.counts[2] == 50 && least.out[0] == 0xA5);
    // every cut: the frames of the two calls together are those of one; each call into a row of its own max_out
    for (size_t cut = 0; cut <= s.size(); cut += (cut < 80 ? 1 : 13))
    {
      st = HdlcState();
      const uint32_t o1 = hdlc_max_out((uint32_t)(cut > 0 ? cut : 1), m, 512), o2 = hdlc_max_out((uint32_t)(s.size() - cut > 0 ? s.size() - cut : 1), m, 512);
      Result a = run(s, 0, cut, lim, &st, o1), b = run(s, cut, s.size(), lim, &st, o2);
      CHECK(a.counts[0] + b.counts[0] == 50 && a.counts[2] + b.counts[2] == 0 && a.counts[1] + b.counts[1] == 0);
      for (uint32_t i = 0; i < 50; i++)
      {
        const uint8_t *rec = i < a.counts[0] ? a.out.data() + i * size : b.out.data() + (i - a.counts[0]) * size;
        CHECK(memcmp(rec + 4, whole.out.data() + i * size + 4, size - 4) == 0);
      }
    }
  }
  return 0;
}

static int check_random_bytes()
{
  uint32_t seed = 12345;
  for (uint32_t P : {1u, 7u, 1021u})
  {
    for (uint32_t carrier = 0; carrier < 2; carrier++)
    {
      const HdlcLimits lim{1, P, carrier};
      HdlcState st = HdlcState();
      for (int call = 0; call < 20; call++)
      {
        std::vector<uint8_t> s(1 + (seed >> 8) % 3000);
        for (uint8_t &v : s)
        {
          seed = seed * 1664525u + 1013904223u;
          v = (uint8_t)(seed >> 24) | (uint8_t)((seed >> 13) % 7 != 0);       // mostly ones: long runs, many flags
        }
        const uint32_t ob = hdlc_max_out((uint32_t)s.size(), 1, P);
        Result r = run(s, 0, s.size(), lim, &st, ob);
        CHECK(r.counts[2] == 0 && st.ones <= 7 && st.n <= hdlc_cap(P));
      }
    }
  }
  return 0;
}

int main()
{
  if (check_the_checks() || check_the_rules() || check_the_cap() || check_the_row_bound_and_the_cuts() || check_random_bytes())
  {
    return 1;
  }
  printf("san_hdlc ok\n");
  return 0;
}
