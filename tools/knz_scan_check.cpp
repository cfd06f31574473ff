// knz_scan_check.cpp -- kz_knz_scan's host code (kanzi_amd/csrc/kz_knz_host.h: knz_scan_host, the rule, the link step) under the
// sanitizers, on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I kanzi_amd/csrc tools/knz_scan_check.cpp -o /tmp/knz_scan_check && /tmp/knz_scan_check
// Every stream is a heap allocation of exactly n bytes, so a read one byte outside src[0 .. n) is reported; the result arrays are
// allocations of exactly cap entries.  Streams are made here: blocks of random bytes behind a block header with its checksum byte.
#include "kz_knz_host.h"
#include <stdlib.h>
#include <memory>
#include <vector>

static long checked = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("knz_scan_check FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); exit(1); } checked++; } while (0)
static uint32_t rnd() { static uint32_t s = 0x2545F491u; s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; }

// a block of len random bytes as the writer frames it for at most 4 transforms: mode, the length in 1 or 2 bytes, the checksum byte
static std::vector<uint8_t> block(int len, uint64_t& W) {
  const int ds = len < 256 ? 1 : 2;
  const uint32_t mode = (uint32_t)(ds - 1) << 5, skip = ((mode << 4) | 0x0F) & 0xFF, HASH = 0x1E35A7BDu;
  W = 8ull * (uint64_t)(2 + ds + len);
  std::vector<uint8_t> b;
  b.push_back((uint8_t)mode);
  if (ds == 2) b.push_back((uint8_t)(len >> 8));
  b.push_back((uint8_t)len);
  uint32_t c = HASH * 0x01030507u;
  c = mix32(c, HASH, mode); c = mix32(c, HASH, skip); c = mix32(c, HASH, (uint32_t)len); c = mix32(c, HASH, (uint32_t)(W >> 32)); c = mix32(c, HASH, (uint32_t)W);
  b.push_back((uint8_t)(((c >> 23) ^ (c >> 3)) & 0xFF));
  for (int i = 0; i < len; i++) b.push_back((uint8_t)rnd());
  return b;
}
struct Stream { std::unique_ptr<uint8_t[]> p; int64_t n; std::vector<int64_t> pre, off, W; };
static Stream stream(const std::vector<int>& lens, bool endMarker = true, int64_t cutBytes = 0) {
  std::vector<uint8_t> tmp(64 + lens.size() * 1100, 0);
  HostBits bs{tmp.data(), (int64_t)tmp.size(), 0, false};
  int64_t total = 0;
  for (int l : lens) total += l;
  write_stream_header(bs, 0, 0, 1024, total, 0);
  Stream s;
  for (int l : lens) {
    uint64_t W;
    const std::vector<uint8_t> b = block(l, W);
    s.pre.push_back((int64_t)bs.pos);
    write_block(bs, b.data(), W);
    s.off.push_back((int64_t)(bs.pos - W)); s.W.push_back((int64_t)W);
  }
  if (endMarker) write_end_marker(bs);
  CHECK(!bs.overflow, "stream buffer");
  s.n = (int64_t)((bs.pos + 7) >> 3) - cutBytes;
  s.p.reset(new uint8_t[(size_t)s.n]);                               // exactly n bytes
  memcpy(s.p.get(), tmp.data(), (size_t)s.n);
  return s;
}
struct Scan { int64_t rc, head; std::vector<int64_t> pre, off, W, next; };
static Scan scan(const Stream& s, int minChain, int64_t cap) {
  Scan r;
  std::unique_ptr<int64_t[]> a(new int64_t[(size_t)cap]), b(new int64_t[(size_t)cap]), c(new int64_t[(size_t)cap]), d(new int64_t[(size_t)cap]);
  r.head = -77;
  r.rc = knz_scan_host(s.p.get(), s.n, minChain, nullptr, nullptr, nullptr, nullptr, nullptr, a.get(), b.get(), c.get(), d.get(), cap, &r.head);
  for (int64_t i = 0; i < std::min(r.rc, cap); i++) { r.pre.push_back(a[i]); r.off.push_back(b[i]); r.W.push_back(c[i]); r.next.push_back(d[i]); }
  return r;
}

int main() {
  // ---- intact streams of 0 .. 40 blocks of 1 .. 1024 bytes: the chain from head is the stream's, END behind it ----
  for (int nb = 0; nb <= 40; nb += (nb < 6 ? 1 : 17)) {
    std::vector<int> lens;
    for (int i = 0; i < nb; i++) lens.push_back(1 + (int)(rnd() % 1024));
    const Stream s = stream(lens);
    for (int mc = 1; mc <= 5; mc += 2) {
      const Scan r = scan(s, mc, 4096);
      CHECK(r.rc >= nb && r.rc <= 4096, "count %lld of %d blocks, minChain %d", (long long)r.rc, nb, mc);
      int64_t i = r.head;
      for (int k = 0; k < nb; k++) {
        CHECK(i >= 0 && i < r.rc && r.pre[i] == s.pre[k] && r.off[i] == s.off[k] && r.W[i] == s.W[k], "block %d of %d, minChain %d", k, nb, mc);
        i = r.next[i];
      }
      CHECK(i == KNZ_SCAN_END, "the end of %d blocks, minChain %d: %lld", nb, mc, (long long)i);
      const Scan part = scan(s, mc, r.rc / 2);                       // a short capacity: the same count, the first entries
      CHECK(part.rc == r.rc && part.head == r.head, "short capacity");
      for (int64_t k = 0; k < r.rc / 2; k++) CHECK(part.pre[k] == r.pre[k] && part.next[k] == r.next[k], "entry %lld under a short capacity", (long long)k);
    }
  }
  // ---- no end marker, and cuts of 1 .. 40 bytes: every read stays inside the n bytes; the whole blocks in front come back ----
  {
    const std::vector<int> lens = {300, 20, 700, 5, 1024, 64, 64, 900};
    for (int64_t cut = 0; cut <= 40; cut++) {
      const Stream s = stream(lens, cut == 0 ? false : true, cut);
      const Scan r = scan(s, 4, 64);
      int64_t i = r.head, k = 0;
      for (; i >= 0; k++) { CHECK(r.pre[i] == s.pre[k] && r.W[i] == s.W[k], "cut %lld, block %lld", (long long)cut, (long long)k); i = r.next[i]; }
      CHECK(i == KNZ_SCAN_BROKEN && k >= 7 && (cut < 2 ? k == 8 : k == 7), "cut %lld: %lld blocks, end %lld", (long long)cut, (long long)k, (long long)i);
    }
  }
  // ---- refusals ----
  {
    const Stream s = stream({100, 200, 300});
    int64_t a[4], head = -77;
    CHECK(knz_scan_host(nullptr, s.n, 4, 0, 0, 0, 0, 0, a, a, a, a, 4, &head) == -KZ_ERR_INVALID_PARAM, "null src");
    CHECK(knz_scan_host(s.p.get(), s.n, 0, 0, 0, 0, 0, 0, a, a, a, a, 4, &head) == -KZ_ERR_INVALID_PARAM, "minChain 0");
    CHECK(knz_scan_host(s.p.get(), -1, 4, 0, 0, 0, 0, 0, a, a, a, a, 4, &head) == -KZ_ERR_INVALID_PARAM, "n < 0");
    CHECK(knz_scan_host(s.p.get(), s.n, 4, 0, 0, 0, 0, 0, a, a, a, a, -1, &head) == -KZ_ERR_INVALID_PARAM, "cap < 0");
    CHECK(knz_scan_host(s.p.get(), s.n, 4, 0, 0, 0, 0, 0, a, a, a, a, 4, nullptr) == -KZ_ERR_INVALID_PARAM, "null head");
    CHECK(knz_scan_host(s.p.get(), 19, 4, 0, 0, 0, 0, 0, a, a, a, a, 4, &head) == -KZ_ERR_INVALID_FILE, "n < 20");
    CHECK(knz_scan_host(s.p.get(), s.n, 4, 0, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, &head) == 3 && head == 0, "cap 0 with null arrays");
  }
  printf("knz_scan_check ok: %ld checks\n", checked);
  return 0;
}
