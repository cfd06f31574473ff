// kz_cm_host.h -- the host-side arithmetic of the CM stage (kz_cm.hip), kept apart so that a plain C++ program can check it
// (tools/cm_host_check.cpp, built with -fsanitize=address,undefined).
#pragma once
#include <stdint.h>
#include <stddef.h>

#define KZ_CM_MAX_BLOCK (1 << 26)              // BinaryEntropyEncoder.java:52 MAX_CHUNK_SIZE: longer blocks are coded in 8 or 16 chunks there

// the varint in front of a payload of sz bytes (EntropyUtils.writeVarInt)
static inline int kz_cm_varint_bytes(uint32_t sz) { int n = 1; while (sz >= 128) { n++; sz >>= 7; } return n; }

// The payload buffer of a block of n bytes: n + n/8 + 1024 rounded up to 256 bytes (whole rows of 64 words), which is
// kz_max_block_stream_bytes(n).  No input built so far comes near it (tests/cmcases.py: the greedy adversary expands by 3.7 %), but
// the coder's worst case is 11 bits per bit, so the cursor is checked and a block that does not fit fails.  k_cm_enc computes the
// same value from the block's length.
static inline int64_t kz_cm_payload_cap(int n) { return (int64_t)(((size_t)n + (size_t)(n >> 3) + 1024 + 255) / 256 * 256); }
