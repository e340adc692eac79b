// Stand-alone robustness harness for the host FLAC decoder (audiotokenization_amd/csrc/flac.cpp), compiled
// together with it by the host compiler (tests/test_flac_harness.py: once plain, once under ASan + UBSan).
// Host code only: it is never loaded into Python and never touches the GPU.
//
//   flac_harness N FLIP.flac [MORE.flac ...]
//
//   1. random mutation: N decodes per stream of an exact-size malloc copy (an over-read is a heap error)
//      with 1-3 bytes overwritten or bits flipped, one run in seven truncated at a random length,
//      int32 / float output and check_crc 0 / 1 in turn, the output buffer exactly channels * cap.
//      The return value is in [0, cap] or one of -1 ... -5.
//   2. every single-bit flip from FLIP's first frame to its end (total known, >= 3 frames, check_crc = 1)
//      returns a negative code.
//   3. every prefix of FLIP (lengths 0 ... n - 1) returns a negative code; length 0 and null arguments
//      return -FLAC_EARG.
//   4. hand-made headers and frames return the stated codes.
// Deterministic (fixed-seed xorshift, no clock).  Exit status 0 = every property held; the first violated
// one is printed (file, offset, values) and the exit status is 1.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

extern "C" int bc_flac_info(const unsigned char*, long long, int*, int*, int*, long long*);
extern "C" long long bc_flac_decode(const unsigned char*, long long, void*, int, long long, int);

namespace {

enum { OK = 0, EARG = 1, ECORRUPT = 2, EUNSUPPORTED = 3, ECRC = 4, ESPACE = 5 };

uint64_t rng_state = 88172645463325252ull;
uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

[[noreturn]] void fail(const std::string& what) {
  printf("FAIL: %s\n", what.c_str());
  fflush(stdout);
  exit(1);
}

std::string fmt(const char* f, ...) __attribute__((format(printf, 1, 2)));
std::string fmt(const char* f, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}

std::vector<uint8_t> slurp(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) fail(fmt("%s: cannot open", path));
  std::vector<uint8_t> d;
  uint8_t buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + n);
  fclose(f);
  if (d.empty()) fail(fmt("%s: empty", path));
  return d;
}

size_t first_frame(const std::vector<uint8_t>& d) {
  size_t pos = 4;
  while (true) {
    if (pos + 4 > d.size()) fail("corpus stream without a last metadata block");
    const bool last = d[pos] & 0x80;
    pos += 4 + (((size_t)d[pos + 1] << 16) | ((size_t)d[pos + 2] << 8) | d[pos + 3]);
    if (last) return pos;
  }
}

// ---- 1. random mutation ----------------------------------------------------------------------------------------
long mutate(const char* name, const std::vector<uint8_t>& d, long N, long* codes) {
  int r, c, b;
  long long total;
  if (bc_flac_info(d.data(), (long long)d.size(), &r, &c, &b, &total) != 0 || total <= 0)
    fail(fmt("%s: the unmutated stream has no readable STREAMINFO with a known total", name));
  {
    std::vector<int32_t> out((size_t)c * total);
    const long long got = bc_flac_decode(d.data(), (long long)d.size(), out.data(), 1, total, 1);
    if (got != total) fail(fmt("%s: the unmutated stream decodes to %lld, not %lld", name, got, total));
  }
  const size_t n = d.size();
  for (long it = 0; it < N; ++it) {
    const size_t m = (it % 7 == 0) ? 1 + rnd() % n : n;
    uint8_t* p = (uint8_t*)malloc(m);
    memcpy(p, d.data(), m);
    const int nm = 1 + (int)(rnd() % 3);
    size_t at[3] = {0, 0, 0};
    for (int k = 0; k < nm; ++k) {
      at[k] = rnd() % m;
      if (it % 3 == 0) p[at[k]] ^= (uint8_t)(1u << (rnd() % 8));
      else p[at[k]] = (uint8_t)rnd();
    }
    int mr, mc, mb;
    long long mt;
    const int irc = bc_flac_info(p, (long long)m, &mr, &mc, &mb, &mt);
    if (irc < 0 || irc > 3) fail(fmt("%s: iteration %ld: bc_flac_info returned %d", name, it, irc));
    if (irc == 0) {
      if (mc < 1 || mc > 8 || mb < 4 || mb > 32 || mr <= 0)
        fail(fmt("%s: iteration %ld: accepted STREAMINFO rate %d channels %d bits %d", name, it, mr, mc, mb));
      const long long cap = (it % 5 == 0) ? total / 3 : total;
      void* out = malloc((size_t)mc * (size_t)cap * 4 + (cap == 0));
      const long long got = bc_flac_decode(p, (long long)m, out, (int)(it & 1), cap, (int)((it >> 1) & 1));
      free(out);
      if (got > cap || got < -5)
        fail(fmt("%s: iteration %ld (length %zu, bytes at %zu %zu %zu): decode returned %lld, cap %lld", name, it, m,
                 at[0], at[1], at[2], got, cap));
      codes[got >= 0 ? 0 : -got]++;
    } else {
      codes[6]++;
    }
    free(p);
  }
  return N;
}

// ---- 2. every single-bit flip ----------------------------------------------------------------------------------
long flips(const char* name, const std::vector<uint8_t>& d0) {
  std::vector<uint8_t> d(d0);
  int r, c, b;
  long long total;
  if (bc_flac_info(d.data(), (long long)d.size(), &r, &c, &b, &total) != 0 || total <= 0)
    fail(fmt("%s: flip stream needs a known total", name));
  const size_t start = first_frame(d);
  uint8_t* p = (uint8_t*)malloc(d.size());
  memcpy(p, d.data(), d.size());
  std::vector<int32_t> out((size_t)c * total);
  long count = 0;
  for (size_t i = start; i < d.size(); ++i)
    for (int bit = 0; bit < 8; ++bit) {
      p[i] ^= (uint8_t)(1u << bit);
      const long long got = bc_flac_decode(p, (long long)d.size(), out.data(), 1, total, 1);
      if (got >= 0 || got < -5) fail(fmt("%s: byte %zu bit %d flipped: decode returned %lld", name, i, bit, got));
      p[i] ^= (uint8_t)(1u << bit);
      ++count;
    }
  free(p);
  return count;
}

// ---- 3. every prefix -------------------------------------------------------------------------------------------
long prefixes(const char* name, const std::vector<uint8_t>& d) {
  int r, c, b;
  long long total;
  bc_flac_info(d.data(), (long long)d.size(), &r, &c, &b, &total);
  std::vector<int32_t> out((size_t)c * total);
  for (size_t m = 0; m < d.size(); ++m) {
    uint8_t* p = (uint8_t*)malloc(m ? m : 1);
    memcpy(p, d.data(), m);
    const long long got = bc_flac_decode(p, (long long)m, out.data(), 1, total, 1);
    int pr, pc, pb;
    long long pt;
    const int irc = bc_flac_info(p, (long long)m, &pr, &pc, &pb, &pt);
    free(p);
    if (got >= 0 || got < -5) fail(fmt("%s: prefix of %zu bytes: decode returned %lld", name, m, got));
    if (m == 0 && (got != -EARG || irc != EARG)) fail(fmt("%s: length 0: %lld / %d, not EARG", name, got, irc));
    if (irc < 0 || irc > 3) fail(fmt("%s: prefix of %zu bytes: info returned %d", name, m, irc));
  }
  const long long n = (long long)d.size();
  if (bc_flac_decode(nullptr, n, out.data(), 1, total, 1) != -EARG) fail("null data: not EARG");
  if (bc_flac_decode(d.data(), n, nullptr, 1, total, 1) != -EARG) fail("null output: not EARG");
  if (bc_flac_decode(d.data(), n, out.data(), 1, -1, 1) != -EARG) fail("negative max_samples: not EARG");
  if (bc_flac_decode(d.data(), -1, out.data(), 1, total, 1) != -EARG) fail("negative length: not EARG");
  if (bc_flac_info(nullptr, n, &r, &c, &b, &total) != EARG) fail("info with null data: not EARG");
  if (bc_flac_info(d.data(), n, nullptr, nullptr, nullptr, nullptr) != OK) fail("info with null outputs: not OK");
  return (long)d.size();
}

// ---- 4. hand-made headers and frames ---------------------------------------------------------------------------
struct BitW {
  std::vector<uint8_t> out;
  int fill = 0;  // bits used in the last byte
  void u(uint64_t v, int n) {
    for (int i = n - 1; i >= 0; --i) {
      if (fill == 0) out.push_back(0);
      out.back() |= (uint8_t)(((v >> i) & 1) << (7 - fill));
      fill = (fill + 1) & 7;
    }
  }
  void s(int64_t v, int n) { u((uint64_t)v & (n >= 64 ? ~0ull : ((1ull << n) - 1)), n); }
  void unary(int q) { u(1, q + 1); }
  void align() { fill = 0; }
};

uint8_t crc8(const uint8_t* d, size_t n) {
  uint8_t c = 0;
  for (size_t i = 0; i < n; ++i) {
    c ^= d[i];
    for (int b = 0; b < 8; ++b) c = (uint8_t)((c & 0x80) ? (c << 1) ^ 0x07 : c << 1);
  }
  return c;
}

uint16_t crc16(const uint8_t* d, size_t n) {
  uint16_t c = 0;
  for (size_t i = 0; i < n; ++i) {
    c ^= (uint16_t)(d[i] << 8);
    for (int b = 0; b < 8; ++b) c = (uint16_t)((c & 0x8000) ? (c << 1) ^ 0x8005 : c << 1);
  }
  return c;
}

struct Info {
  int min_block = 16, max_block = 16, rate = 16000, channels = 1, bits = 16;
  uint64_t total = 0;
};

std::vector<uint8_t> streaminfo(const Info& si) {
  BitW w;
  w.u(si.min_block, 16);
  w.u(si.max_block, 16);
  w.u(0, 24);
  w.u(0, 24);
  w.u(si.rate, 20);
  w.u(si.channels - 1, 3);
  w.u(si.bits - 1, 5);
  w.u(si.total, 36);
  for (int i = 0; i < 4; ++i) w.u(0, 32);
  return w.out;
}

void block(std::vector<uint8_t>& d, int type, bool last, const std::vector<uint8_t>& body, long claimed = -1) {
  const size_t len = claimed < 0 ? body.size() : (size_t)claimed;
  d.push_back((uint8_t)((last ? 0x80 : 0) | type));
  d.push_back((uint8_t)(len >> 16));
  d.push_back((uint8_t)(len >> 8));
  d.push_back((uint8_t)len);
  d.insert(d.end(), body.begin(), body.end());
}

std::vector<uint8_t> head(const Info& si) {
  std::vector<uint8_t> d = {'f', 'L', 'a', 'C'};
  block(d, 0, true, streaminfo(si));
  return d;
}

struct Frame {
  int reserved1 = 0, bs = 16, src = 5, chc = 0, ssc = 4, reserved2 = 0;
  int bsc = -1;  // -1: code 6 with bs - 1 in one byte
};

// one frame: the header with a correct CRC-8, the subframes `body` writes, padding, a correct CRC-16
void frame(std::vector<uint8_t>& d, const Frame& f, const std::function<void(BitW&)>& body) {
  BitW w;
  w.u(0x3FFE, 14);
  w.u(f.reserved1, 1);
  w.u(0, 1);
  w.u(f.bsc < 0 ? 6 : f.bsc, 4);
  w.u(f.src, 4);
  w.u(f.chc, 4);
  w.u(f.ssc, 3);
  w.u(f.reserved2, 1);
  w.u(0, 8);  // frame number 0
  if (f.bsc < 0) w.u(f.bs - 1, 8);
  w.u(crc8(w.out.data(), w.out.size()), 8);
  body(w);
  w.align();
  const uint16_t c = crc16(w.out.data(), w.out.size());
  w.u(c, 16);
  d.insert(d.end(), w.out.begin(), w.out.end());
}

void sub_header(BitW& w, int type, int wasted = 0) {
  w.u(0, 1);
  w.u(type, 6);
  if (wasted) {
    w.u(1, 1);
    w.unary(wasted - 1);
  } else {
    w.u(0, 1);
  }
}

void verbatim(BitW& w, int bs, int bps, int64_t v) {
  sub_header(w, 1);
  for (int i = 0; i < bs; ++i) w.s(v, bps);
}

// residual of `cnt` samples in one escaped partition of `nb` bits (partition order `porder`, first partition only)
void escaped(BitW& w, int porder, int nb, int cnt, int64_t v) {
  w.u(0, 2);
  w.u(porder, 4);
  w.u(15, 4);
  w.u(nb, 5);
  for (int i = 0; i < cnt; ++i) w.s(v, nb);
}

int n_cases = 0;

void expect(const char* what, const std::vector<uint8_t>& d, long long want, int info_want = -1) {
  uint8_t* p = (uint8_t*)malloc(d.size());
  memcpy(p, d.data(), d.size());
  int r = 0, c = 0, b = 0;
  long long t = 0;
  const int irc = bc_flac_info(p, (long long)d.size(), &r, &c, &b, &t);
  if (info_want >= 0 && irc != info_want) fail(fmt("hand-made '%s': info returned %d, expected %d", what, irc, info_want));
  const int ch = (irc == 0 && c >= 1 && c <= 8) ? c : 8;
  for (int mode = 0; mode < 4; ++mode) {  // int32 / float x check_crc 0 / 1
    std::vector<int32_t> out((size_t)ch * 64);
    const long long got = bc_flac_decode(p, (long long)d.size(), out.data(), mode & 1, 64, mode >> 1);
    if (got != want) fail(fmt("hand-made '%s' (mode %d): decode returned %lld, expected %lld", what, mode, got, want));
  }
  free(p);
  ++n_cases;
}

void handmade() {
  const Info mono;
  // -- metadata
  {
    std::vector<uint8_t> d = {'f', 'L', 'a', 'C'};
    std::vector<uint8_t> si = streaminfo(mono);
    si.resize(33);
    block(d, 0, true, si);
    expect("STREAMINFO of 33 bytes", d, -ECORRUPT, ECORRUPT);
  }
  {
    std::vector<uint8_t> d = {'f', 'L', 'a', 'C'};
    block(d, 0, false, streaminfo(mono));
    block(d, 127, true, std::vector<uint8_t>(4));
    expect("metadata block type 127", d, -ECORRUPT, ECORRUPT);
  }
  {
    std::vector<uint8_t> d = {'f', 'L', 'a', 'C'};
    block(d, 0, false, streaminfo(mono));
    block(d, 1, true, std::vector<uint8_t>(10), 11);
    expect("metadata length past the end", d, -ECORRUPT, ECORRUPT);
  }
  {
    std::vector<uint8_t> d = {'f', 'L', 'a', 'C'};
    block(d, 0, true, streaminfo(mono), 0xFFFFFF);
    expect("STREAMINFO length past the end", d, -ECORRUPT, ECORRUPT);
  }
  {
    std::vector<uint8_t> d = {'f', 'L', 'a', 'C'};
    block(d, 1, true, std::vector<uint8_t>(40));
    frame(d, Frame(), [](BitW& w) { verbatim(w, 16, 16, 5); });
    expect("no STREAMINFO", d, -ECORRUPT, ECORRUPT);
  }
  {
    std::vector<uint8_t> d = {'f', 'L', 'a', 'C'};
    block(d, 0, false, streaminfo(mono));  // no block is marked last
    expect("metadata without a last block", d, -ECORRUPT, ECORRUPT);
  }
  {
    std::vector<uint8_t> d = {'f', 'L', 'a', 'X'};
    block(d, 0, true, streaminfo(mono));
    expect("wrong magic", d, -ECORRUPT, ECORRUPT);
  }
  for (int which = 0; which < 3; ++which) {
    Info si;
    if (which == 0) si.bits = 3;
    if (which == 1) si.rate = 0;
    if (which == 2) si.max_block = si.min_block = 15;
    std::vector<uint8_t> d = head(si);
    Frame f;
    f.ssc = 0;
    f.src = 0;
    frame(d, f, [&](BitW& w) { verbatim(w, 16, si.bits, 1); });
    expect(which == 0 ? "3-bit samples" : which == 1 ? "rate 0" : "maximum block size 15", d, -ECORRUPT, ECORRUPT);
  }
  // -- the makers themselves: a good stream decodes (one VERBATIM frame; a FIXED and an LPC frame at the range's edge)
  {
    std::vector<uint8_t> d = head(mono);
    frame(d, Frame(), [](BitW& w) { verbatim(w, 16, 16, -1234); });
    expect("good VERBATIM frame", d, 16, OK);
    int32_t out[16];
    bc_flac_decode(d.data(), (long long)d.size(), out, 1, 16, 1);
    for (int i = 0; i < 16; ++i)
      if (out[i] != -1234) fail(fmt("good VERBATIM frame: sample %d is %d", i, out[i]));
  }
  {
    std::vector<uint8_t> d = head(mono);
    frame(d, Frame(), [](BitW& w) {  // FIXED order 1 from 32766, residuals +1 then 0: ends at 32767, the last value
      sub_header(w, 9);
      w.s(32766, 16);
      w.u(0, 2);
      w.u(0, 4);
      w.u(15, 4);
      w.u(2, 5);
      w.s(1, 2);
      for (int i = 0; i < 14; ++i) w.s(0, 2);
    });
    expect("FIXED order 1 reaching 32767", d, 16, OK);
    int32_t out[16];
    bc_flac_decode(d.data(), (long long)d.size(), out, 1, 16, 1);
    if (out[0] != 32766 || out[1] != 32767 || out[15] != 32767) fail("FIXED order 1 reaching 32767: wrong samples");
  }
  {
    std::vector<uint8_t> d = head(mono);
    frame(d, Frame(), [](BitW& w) {  // LPC order 1, coefficient 1 >> 0, from -32768 with residual 0: stays at the edge
      sub_header(w, 32);
      w.s(-32768, 16);
      w.u(1, 4);  // precision 2
      w.s(0, 5);
      w.s(1, 2);
      escaped(w, 0, 0, 15, 0);
    });
    expect("LPC order 1 holding -32768", d, 16, OK);
    int32_t out[16];
    bc_flac_decode(d.data(), (long long)d.size(), out, 1, 16, 1);
    if (out[0] != -32768 || out[15] != -32768) fail("LPC order 1 holding -32768: wrong samples");
  }
  // -- frame header
  {
    Info si;
    std::vector<uint8_t> d = head(si);
    Frame f;
    f.chc = 1;
    frame(d, f, [](BitW& w) {
      verbatim(w, 16, 16, 1);
      verbatim(w, 16, 16, 1);
    });
    expect("2-channel frame in a mono stream", d, -ECORRUPT, OK);
  }
  {
    Info si;
    si.channels = 2;
    std::vector<uint8_t> d = head(si);
    frame(d, Frame(), [](BitW& w) { verbatim(w, 16, 16, 1); });
    expect("mono frame in a stereo stream", d, -ECORRUPT, OK);
  }
  {
    std::vector<uint8_t> d = head(mono);
    Frame f;
    f.chc = 11;
    frame(d, f, [](BitW& w) { verbatim(w, 16, 16, 1); });
    expect("reserved channel assignment 11", d, -ECORRUPT, OK);
  }
  {
    std::vector<uint8_t> d = head(mono);
    Frame f;
    f.bsc = 0;
    frame(d, f, [](BitW& w) { verbatim(w, 16, 16, 1); });
    expect("block-size code 0", d, -ECORRUPT, OK);
  }
  {
    std::vector<uint8_t> d = head(mono);
    Frame f;
    f.src = 15;
    frame(d, f, [](BitW& w) { verbatim(w, 16, 16, 1); });
    expect("sample-rate code 15", d, -ECORRUPT, OK);
  }
  {
    std::vector<uint8_t> d = head(mono);
    Frame f;
    f.ssc = 3;
    frame(d, f, [](BitW& w) { verbatim(w, 16, 16, 1); });
    expect("sample-size code 3", d, -ECORRUPT, OK);
  }
  {
    std::vector<uint8_t> d = head(mono);
    Frame f;
    f.reserved1 = 1;
    frame(d, f, [](BitW& w) { verbatim(w, 16, 16, 1); });
    expect("reserved bit after the sync code set", d, -ECORRUPT, OK);
  }
  {
    Info si;
    si.total = 32;
    std::vector<uint8_t> d = head(si);
    frame(d, Frame(), [](BitW& w) { verbatim(w, 16, 16, 1); });
    Frame f;
    f.reserved1 = 1;
    frame(d, f, [](BitW& w) { verbatim(w, 16, 16, 1); });
    expect("reserved bit after the sync code set in the second frame", d, -ECORRUPT, OK);
  }
  {
    std::vector<uint8_t> d = head(mono);
    Frame f;
    f.reserved2 = 1;
    frame(d, f, [](BitW& w) { verbatim(w, 16, 16, 1); });
    expect("reserved bit after the sample size set", d, -ECORRUPT, OK);
  }
  for (int ssc : {1, 2, 5, 6, 7}) {  // 8 / 12 / 20 / 24 / 32-bit frames in a 16-bit stream
    static const int bits[8] = {0, 8, 12, 0, 16, 20, 24, 32};
    std::vector<uint8_t> d = head(mono);
    Frame f;
    f.ssc = ssc;
    frame(d, f, [&](BitW& w) { verbatim(w, 16, bits[ssc], 1); });
    expect("frame sample size differs from STREAMINFO", d, -EUNSUPPORTED, OK);
  }
  {
    Info si;
    si.bits = 24;
    std::vector<uint8_t> d = head(si);
    frame(d, Frame(), [](BitW& w) { verbatim(w, 16, 16, 1); });  // a 16-bit frame in a 24-bit stream
    expect("16-bit frame in a 24-bit stream", d, -EUNSUPPORTED, OK);
  }
  // -- subframes
  {
    std::vector<uint8_t> d = head(mono);
    Frame f;
    f.bs = 17;
    frame(d, f, [](BitW& w) {
      sub_header(w, 8);
      w.u(0, 2);
      w.u(1, 4);  // two partitions of a 17-sample block
      for (int pt = 0; pt < 2; ++pt) {
        w.u(15, 4);
        w.u(0, 5);
      }
    });
    expect("partition order that does not divide the block", d, -ECORRUPT, OK);
  }
  {
    std::vector<uint8_t> d = head(mono);
    frame(d, Frame(), [](BitW& w) {
      sub_header(w, 10);  // FIXED order 2
      w.s(0, 16);
      w.s(0, 16);
      w.u(0, 2);
      w.u(4, 4);  // 16 partitions of 1 sample: less than the order
      for (int pt = 0; pt < 16; ++pt) {
        w.u(15, 4);
        w.u(0, 5);
      }
    });
    expect("partition shorter than the predictor order", d, -ECORRUPT, OK);
  }
  {
    std::vector<uint8_t> d = head(mono);
    Frame f;
    f.bs = 2;
    frame(d, f, [](BitW& w) {
      sub_header(w, 12);
      for (int i = 0; i < 4; ++i) w.s(0, 16);
      escaped(w, 0, 0, 0, 0);
    });
    expect("FIXED order 4 in a block of 2", d, -ECORRUPT, OK);
  }
  {
    std::vector<uint8_t> d = head(mono);
    frame(d, Frame(), [](BitW& w) {
      sub_header(w, 63);  // LPC order 32 in a block of 16
      for (int i = 0; i < 32; ++i) w.s(0, 16);
      w.u(1, 4);
      w.s(0, 5);
      for (int i = 0; i < 32; ++i) w.s(0, 2);
      escaped(w, 0, 0, 0, 0);
    });
    expect("LPC order 32 in a block of 16", d, -ECORRUPT, OK);
  }
  for (int type : {2, 7, 13, 31}) {
    std::vector<uint8_t> d = head(mono);
    frame(d, Frame(), [&](BitW& w) {
      sub_header(w, type);
      for (int i = 0; i < 16; ++i) w.s(0, 16);
    });
    expect("reserved subframe type", d, -ECORRUPT, OK);
  }
  {
    std::vector<uint8_t> d = head(mono);
    frame(d, Frame(), [](BitW& w) {
      w.u(1, 1);  // the subframe's padding bit
      w.u(1, 6);
      w.u(0, 1);
      for (int i = 0; i < 16; ++i) w.s(0, 16);
    });
    expect("subframe padding bit set", d, -ECORRUPT, OK);
  }
  {
    std::vector<uint8_t> d = head(mono);
    frame(d, Frame(), [](BitW& w) {
      sub_header(w, 1, 16);  // 16 wasted bits of 16
      for (int i = 0; i < 16; ++i) w.s(0, 16);
    });
    expect("as many wasted bits as sample bits", d, -ECORRUPT, OK);
  }
  {
    std::vector<uint8_t> d = head(mono);
    frame(d, Frame(), [](BitW& w) {
      sub_header(w, 8);
      w.u(2, 2);  // reserved residual coding method
      w.u(0, 4);
      for (int i = 0; i < 16; ++i) w.u(0xFFFF, 16);
    });
    expect("reserved residual coding method", d, -ECORRUPT, OK);
  }
  {
    std::vector<uint8_t> d = head(mono);
    frame(d, Frame(), [](BitW& w) {
      sub_header(w, 32);
      w.s(0, 16);
      w.u(15, 4);  // precision code 15
      w.s(0, 5);
      w.s(0, 16);
      escaped(w, 0, 0, 15, 0);
    });
    expect("LPC precision code 15", d, -ECORRUPT, OK);
  }
  {
    std::vector<uint8_t> d = head(mono);
    frame(d, Frame(), [](BitW& w) {
      sub_header(w, 32);
      w.s(0, 16);
      w.u(1, 4);
      w.s(-1, 5);  // negative shift
      w.s(1, 2);
      escaped(w, 0, 0, 15, 0);
    });
    expect("negative LPC shift", d, -EUNSUPPORTED, OK);
  }
  // -- restored samples that leave their range
  {
    std::vector<uint8_t> d = head(mono);
    frame(d, Frame(), [](BitW& w) {  // FIXED order 1 from 32767 with residual +1
      sub_header(w, 9);
      w.s(32767, 16);
      escaped(w, 0, 2, 15, 1);
    });
    expect("FIXED order 1 leaving the 16-bit range", d, -ECORRUPT, OK);
  }
  {
    std::vector<uint8_t> d = head(mono);
    frame(d, Frame(), [](BitW& w) {  // FIXED order 4 on an alternating full-scale history: 16 x 32768 predicted
      sub_header(w, 12);
      for (int i = 0; i < 4; ++i) w.s(i & 1 ? -32768 : 32767, 16);
      escaped(w, 0, 0, 12, 0);
    });
    expect("FIXED order 4 leaving the 16-bit range", d, -ECORRUPT, OK);
  }
  {
    std::vector<uint8_t> d = head(mono);
    frame(d, Frame(), [](BitW& w) {  // Rice parameter 30 and a quotient of 40: residuals of 36 bits
      sub_header(w, 12);
      for (int i = 0; i < 4; ++i) w.s(i & 1 ? -32768 : 32767, 16);
      w.u(1, 2);
      w.u(0, 4);
      w.u(30, 5);
      for (int i = 0; i < 12; ++i) {
        w.unary(40);
        w.u(0x3FFFFFFF, 30);
      }
    });
    expect("FIXED order 4 with residuals of 36 bits", d, -ECORRUPT, OK);
  }
  {
    std::vector<uint8_t> d = head(mono);
    frame(d, Frame(), [](BitW& w) {  // LPC order 1, coefficient 16383 >> 0, from 32767
      sub_header(w, 32);
      w.s(32767, 16);
      w.u(14, 4);  // precision 15
      w.s(0, 5);
      w.s(16383, 15);
      escaped(w, 0, 0, 15, 0);
    });
    expect("LPC order 1 leaving the 16-bit range", d, -ECORRUPT, OK);
  }
  {
    Info si;
    si.bits = 32;
    std::vector<uint8_t> d = head(si);
    Frame f;
    f.ssc = 7;
    f.bs = 64;
    frame(d, f, [](BitW& w) {  // LPC order 32 of full-scale 32-bit samples and full-scale 15-bit coefficients: 2^50
      sub_header(w, 63);
      for (int i = 0; i < 32; ++i) w.s(INT32_MIN, 32);
      w.u(14, 4);
      w.s(0, 5);
      for (int i = 0; i < 32; ++i) w.s(-16384, 15);
      escaped(w, 0, 31, 32, -(1 << 30));
    });
    expect("LPC order 32 at full scale leaving the 32-bit range", d, -ECORRUPT, OK);
  }
  for (int chc : {8, 9, 10}) {
    Info si;
    si.channels = 2;
    std::vector<uint8_t> d = head(si);
    Frame f;
    f.chc = chc;
    frame(d, f, [&](BitW& w) {
      // left / side: right = -32768 - 65535; side / right: left = -65536 + -32768; mid / side: left = 65535
      if (chc == 8) {
        verbatim(w, 16, 16, -32768);
        verbatim(w, 16, 17, 65535);
      } else if (chc == 9) {
        verbatim(w, 16, 17, -65536);
        verbatim(w, 16, 16, -32768);
      } else {
        verbatim(w, 16, 16, 32767);
        verbatim(w, 16, 17, 65535);
      }
    });
    expect("decorrelated channel leaving the 16-bit range", d, -ECORRUPT, OK);
  }
  {
    Info si;
    si.channels = 2;
    si.bits = 32;
    std::vector<uint8_t> d = head(si);
    Frame f;
    f.chc = 8;
    f.ssc = 7;
    frame(d, f, [](BitW& w) {  // 33-bit side: right = INT32_MIN - (2^32 - 1)
      verbatim(w, 16, 32, INT32_MIN);
      verbatim(w, 16, 33, 0xFFFFFFFFll);
    });
    expect("decorrelated channel leaving the 32-bit range", d, -ECORRUPT, OK);
  }
  // -- frames that end early, and trailing bytes
  {
    std::vector<uint8_t> d = head(mono);
    frame(d, Frame(), [](BitW& w) { verbatim(w, 16, 16, 1); });
    d.resize(d.size() - 1);
    expect("frame CRC-16 cut short", d, -ECORRUPT, OK);
  }
  {
    std::vector<uint8_t> d = head(mono);
    expect("no frame at all", d, 0, OK);
  }
  {
    std::vector<uint8_t> d = head(mono);
    d.insert(d.end(), 8, 0x55);
    expect("bytes that are no frame after the metadata", d, -ECORRUPT, OK);
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s N FLIP.flac [MORE.flac ...]\n", argv[0]);
    return 2;
  }
  const long N = atol(argv[1]);
  handmade();
  printf("hand-made: %d cases\n", n_cases);
  const std::vector<uint8_t> flip = slurp(argv[2]);
  printf("single-bit flips: %ld, none accepted\n", flips(argv[2], flip));
  printf("prefixes: %ld, none accepted\n", prefixes(argv[2], flip));
  long codes[7] = {0, 0, 0, 0, 0, 0, 0}, decodes = 0;
  for (int a = 2; a < argc; ++a) decodes += mutate(argv[a], slurp(argv[a]), N, codes);
  printf("mutations: %ld decodes of %d streams: accepted %ld, corrupt %ld, unsupported %ld, crc %ld, space %ld, "
         "header rejected %ld\n", decodes, argc - 2, codes[0], codes[2], codes[3], codes[4], codes[5], codes[6]);
  return 0;
}
