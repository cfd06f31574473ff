// cm_host_check.cpp -- the host-side arithmetic of the CM stage (kanzi_amd/csrc/kz_cm_host.h) under the sanitizers, on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I kanzi_amd/csrc tools/cm_host_check.cpp -o /tmp/cm_host_check && /tmp/cm_host_check
// The varint length against a byte-by-byte writer (EntropyUtils.writeVarInt) at every power-of-128 seam, the payload bound against the
// stride rule of include/kanzi_hip.h (n + n/8 + 1024 rounded up to 256) up to the largest block CM takes, and no overflow on the way.
#include "kz_cm_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static int write_varint(std::vector<uint8_t>& out, uint32_t v) {
  int n = 0;
  while (v >= 128) { out.push_back((uint8_t)(0x80 | (v & 0x7F))); v >>= 7; n++; }
  out.push_back((uint8_t)v);
  return n + 1;
}

int main() {
  long checked = 0;
  const uint32_t seams[] = {0u, 1u, 127u, 128u, 129u, 16383u, 16384u, 16385u, 2097151u, 2097152u, 268435455u, 268435456u, 0x7FFFFFFFu, 0xFFFFFFFFu};
  for (uint32_t v : seams) {
    std::vector<uint8_t> buf;
    const int n = write_varint(buf, v);
    if (n != kz_cm_varint_bytes(v) || (size_t)n != buf.size() || n > 5) { printf("varint length of %u: %d vs %d\n", v, kz_cm_varint_bytes(v), n); return 1; }
    checked++;
  }
  int prev = -1;
  for (int64_t n = 0; n < KZ_CM_MAX_BLOCK; n += (n < 70000 ? 1 : 4099)) {
    const int64_t cap = kz_cm_payload_cap((int)n);
    const int64_t want = (n + n / 8 + 1024 + 255) / 256 * 256;
    if (cap != want || (cap & 255) || cap < n + n / 8 + 1024 || cap >= n + n / 8 + 1024 + 256 || cap < prev) { printf("payload cap of %lld: %lld\n", (long long)n, (long long)cap); return 1; }
    if (6 + kz_cm_varint_bytes((uint32_t)cap) + cap + 7 > 0x7FFFFFFFLL) { printf("row bytes of %lld\n", (long long)n); return 1; }   // header, varint, payload, tail: an int
    prev = (int)cap;
    checked++;
  }
  const int64_t top = kz_cm_payload_cap(KZ_CM_MAX_BLOCK - 1);
  if (top != ((int64_t)KZ_CM_MAX_BLOCK - 1 + ((KZ_CM_MAX_BLOCK - 1) >> 3) + 1024 + 255) / 256 * 256) { printf("payload cap at the limit: %lld\n", (long long)top); return 1; }
  printf("cm_host_check ok: %ld values\n", checked + 1);
  return 0;
}
