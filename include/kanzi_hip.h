/*
 * kanzi_hip.h -- C-ABI of libkanzi_hip.so: the MI355X (gfx950) implementation of Kanzi's per-block
 * hot path.  Plain pointers and sizes only; no C++ or torch types cross this boundary.
 *
 * What each entry point replaces in the reference (K/ = java/src/main/java/io/github/flanglet/kanzi/):
 *
 *   kz_transform_forward / _inverse / _max_encoded_len
 *       K/ByteTransform.java:36,48,56  (boolean forward(SliceByteArray,SliceByteArray), inverse, getMaxEncodedLength)
 *       for the codecs K/transform/BWTBlockCodec.java:71-213, K/transform/SBRT.java:87-214 (RANK, MTFT),
 *       K/transform/ZRLT.java:54-233, K/transform/RLT.java:69-410, K/transform/SRT.java:66-257, K/transform/LZCodec.java:299-756 (LZ, LZX), :1023-1286 (LZP), K/transform/EXECodec.java:110-772 (EXE),
 *       K/transform/FSDCodec.java:60-323 (MM), K/transform/AliasCodec.java:76-475 (PACK, DNA), and, as host (CPU) stages in front of
 *       the GPU chain, K/transform/TextCodec.java:482-531 (TEXT) and K/transform/UTFCodec.java:68-305 (UTF).
 *       "false" is a normal outcome (Sequence.java:95-105) -> return 0.
 *       RLT is built with the context map, as TransformFactory does (new RLT(ctx)): its forward reads the entries "entropy"
 *       (kz_ctx_set_entropy: the escape symbol is searched and the block's data type looked at under every coder but NONE / ANS0 /
 *       HUFFMAN / RANGE, RLT.java:101-132) and "dataType" (kz_ctx_set_data_type; DNA / BASE64 / UTF8 decline, a detected type is
 *       stored back: kz_ctx_get_data_type).  It bounds its output by dst.length, the length of the output ARRAY (RLT.java:115):
 *         kz_transform_forward   dst.length = dstCap (a binding passes the array's length behind dst.index, not the slice's);
 *         batched / stream calls dst.length = what the reference's writer with one job and equal block sizes gives the stage.
 *                                Sequence.forward swaps its two buffers after every stage that was APPLIED (Sequence.java:107-114).
 *                                After an even number of applied stages (host stages TEXT / UTF included) RLT writes into the task's
 *                                `buffer`: Sequence.getMaxEncodedLength(blockSize) bytes (CompressedOutputStream.java:793,806-811);
 *                                after an odd number into `data`: max(blockSize + blockSize / 8, 256 KiB) bytes (:215-216, or what
 *                                the stage needs if that is more, Sequence.java:82-87).  blockSize = kz_ctx_set_block_size when set
 *                                (kz_compress sets it), else the longest block of the call.
 *       The bound only matters for a block whose coded length ends within a few bytes under its length.
 *   kz_entropy_encode / kz_entropy_decode
 *       K/EntropyEncoder.java:34 (int encode(byte[],int,int)) + dispose(), K/EntropyDecoder.java:33
 *       for K/entropy/ANSRangeEncoder.java:263-305, K/entropy/ANSRangeDecoder.java:189-236 (order 0 = ANS0 and
 *       order 1 = ANS1, K/entropy/EntropyCodecFactory.java:124-128,175-179),
 *       K/entropy/HuffmanEncoder.java:380-416, K/entropy/HuffmanDecoder.java:353-390,
 *       K/entropy/FPAQEncoder.java:128-238, K/entropy/FPAQDecoder.java:161-335,
 *       K/entropy/RangeEncoder.java:244-316, K/entropy/RangeDecoder.java:161-327,
 *       K/entropy/NullEntropyEncoder.java:66-81.  The codec's output is a bit string (MSB first,
 *       K/bitstream/DefaultOutputBitStream.java:103-123): the Java adapter calls
 *       obs.writeBits(out, 0, nbits) once.
 *   kz_encode_blocks / kz_decode_blocks  (batched, the form in which the GPU pays off)
 *       the span transform.forward ... ee.dispose of EncodingTask.encodeBlock
 *       (K/io/CompressedOutputStream.java:792-985) resp. ed.decode ... transform.inverse of
 *       DecodingTask.decodeBlock (K/io/CompressedInputStream.java:1286-1344), including the block
 *       header (mode / skipFlags / postTransformLength / header checksum, :861-896,:977-985) and the
 *       raw "transformed copy" fallback (:926-973).  Output per block = the block's private
 *       byte-aligned stream of `bits` bits, ready for the ordered emission loop (:1024-1035).
 *
 * Return convention: >= 0 success (meaning documented per call); negative = -(K/Error.java code).
 * A kz_ctx is single-threaded (one HIP stream, one scratch arena); use one per host thread / GPU,
 * exactly like the reference creates one codec instance per task (CompressedOutputStream.java:792,907).
 */
#ifndef KANZI_HIP_H
#define KANZI_HIP_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KZ_ABI_VERSION 3

/* transform ids: K/transform/TransformFactory.java:36-60 */
enum { KZ_T_NONE = 0, KZ_T_BWT = 1, KZ_T_LZ = 3, KZ_T_RLT = 5, KZ_T_ZRLT = 6, KZ_T_MTFT = 7, KZ_T_RANK = 8, KZ_T_EXE = 9, KZ_T_TEXT = 10 /* DICT_TYPE */,
       KZ_T_SRT = 13, KZ_T_LZP = 14, KZ_T_MM = 15, KZ_T_LZX = 16, KZ_T_UTF = 17, KZ_T_PACK = 18, KZ_T_DNA = 19 };
/* Global.DataType (K/Global.java:40-80): the per-block context entry "dataType" that MM (FSDCodec.java:78-85,160-168),
   LZ/LZX (LZCodec.java:343-352), RLT (RLT.java:95-132) and EXE (EXECodec.java:130-137,156-157) read and write.  The KZ_DT_* VALUES ARE THIS LIBRARY'S OWN and are NOT the Java enum's
   ordinals (Java order: UNDEFINED, TEXT, MULTIMEDIA, EXE, NUMERIC, BASE64, DNA, BIN, UTF8, SMALL_ALPHABET); the value never
   reaches the stream, and a binding maps by NAME (integration/java/HipByteTransform.java). */
enum { KZ_DT_UNDEFINED = 0, KZ_DT_DNA = 1, KZ_DT_SMALL_ALPHABET = 2, KZ_DT_TEXT = 3, KZ_DT_MULTIMEDIA = 4, KZ_DT_EXE = 5,
       KZ_DT_NUMERIC = 6, KZ_DT_BASE64 = 7, KZ_DT_BIN = 8, KZ_DT_UTF8 = 9 };
/* entropy ids: K/entropy/EntropyCodecFactory.java (ANS1_TYPE = 8: order-1 ANS, 4 MiB chunks).  An ANS1 stream carries up to 256
   context headers per chunk: kz_entropy_encode may need more than kz_max_block_stream_bytes(n) for it (n + n/8 + 1024 + 102400
   per started 4 MiB is always enough); the batched calls store such a block as a raw copy, as the reference does (:926-973). */
/* KZ_E_RANGE = RANGE_TYPE 4: K/entropy/RangeEncoder.java:244-316, K/entropy/RangeDecoder.java:161-327 as EntropyCodecFactory builds
   them (32 KiB chunks, logRange 12).  Its frequencies come from each chunk's own histogram, so real data codes below 8.1 bits per
   byte and fits kz_max_block_stream_bytes(n); the coder's worst case is 12 bits per byte and more, so kz_entropy_encode sizes its
   own buffer by the encoder's payload bound (50 KiB per started 32 KiB) and returns KZ_ERR_WRITE_FILE when the caller's is too
   small; the batched calls store such a block as a raw copy, as the reference does (:926-973).  A chunk that outgrows even that
   bound fails its block with KZ_ERR_PROCESS_BLOCK. */
/* KZ_E_CM = CM_TYPE 6: K/entropy/CMPredictor.java:100-186 behind K/entropy/BinaryEntropyEncoder.java:117-155, :187-218, :250-255 and
   K/entropy/BinaryEntropyDecoder.java:117-167, :196-239, one coder and one fresh predictor per block.  Blocks of 1 << 26 bytes and
   more, which the reference codes in 8 or 16 chunks, are refused with KZ_ERR_INVALID_CODEC in both directions.  A block's stream
   (varint, payload, 7-byte tail) must fit what its block header leaves of the output row and a payload buffer of
   kz_max_block_stream_bytes(n) bytes; no input known comes near that (the worst found expands by 3.7 %), but the coder's worst
   case is 11 bits per bit, so the encoder checks, and a block that does not fit fails with KZ_ERR_PROCESS_BLOCK, its row
   untouched behind the header bytes. */
enum { KZ_E_NONE = 0, KZ_E_HUFFMAN = 1, KZ_E_FPAQ = 2, KZ_E_RANGE = 4, KZ_E_ANS0 = 5, KZ_E_CM = 6, KZ_E_ANS1 = 8 };
/* error codes: K/Error.java:24-43 (returned negated); KZ_ERR_DEVICE is the one code the reference has no equivalent for */
enum { KZ_ERR_MISSING_PARAM = 1, KZ_ERR_BLOCK_SIZE = 2, KZ_ERR_INVALID_CODEC = 3, KZ_ERR_READ_FILE = 11,
       KZ_ERR_WRITE_FILE = 12, KZ_ERR_PROCESS_BLOCK = 13, KZ_ERR_INVALID_FILE = 15, KZ_ERR_STREAM_VERSION = 16,
       KZ_ERR_INVALID_PARAM = 18, KZ_ERR_CRC_CHECK = 19, KZ_ERR_DEVICE = 126, KZ_ERR_UNKNOWN = 127 };

/* pointer location flags for the batched calls */
enum { KZ_MEM_HOST = 0, KZ_MEM_DEVICE = 1 };

#define KZ_MAX_STAGES 16
enum { KZ_STAGE_BWT_FWD = 0, KZ_STAGE_SBRT_FWD = 1, KZ_STAGE_ZRLT_FWD = 2, KZ_STAGE_ENTROPY_ENC = 3,
       KZ_STAGE_FRAME_ENC = 4, KZ_STAGE_ENTROPY_DEC = 5, KZ_STAGE_ZRLT_INV = 6, KZ_STAGE_SBRT_INV = 7,
       KZ_STAGE_BWT_INV = 8, KZ_STAGE_FRAME_DEC = 9, KZ_STAGE_LZ_FWD = 10, KZ_STAGE_LZ_INV = 11,
       KZ_STAGE_SRT_FWD = 12, KZ_STAGE_SRT_INV = 13, KZ_STAGE_HOST_FWD = 14, KZ_STAGE_HOST_INV = 15 };

typedef struct kz_ctx kz_ctx;

int32_t     kz_abi_version(void);
kz_ctx*     kz_ctx_create(int32_t deviceId);          /* NULL if no HIP device / out of memory */
void        kz_ctx_destroy(kz_ctx* ctx);
const char* kz_last_error(kz_ctx* ctx);
/* per-block checksum of the original data: bits = 0 (none), 32 (XXHash32) or 64 (XXHash64): the "checksum" key of
 * the reference's context map (K/io/CompressedOutputStream.java:190-204, :749-755, :887-891). Applies to the
 * following kz_encode_blocks / kz_decode_blocks / kz_compress calls (kz_decompress reads it from the stream). */
int32_t     kz_ctx_set_checksum(kz_ctx* ctx, int32_t bits);
/* the "dataType" key of the context map a transform instance is built with (KZ_DT_*): kz_transform_forward reads it
 * the way FSDCodec.forward / LZCodec.forward do (FSDCodec.java:78-85, LZCodec.java:343-352) and stores back what the
 * reference would store (FSDCodec.java:160-168).  The batched calls tag every block themselves, like the writer does
 * from the block's first four bytes (K/Magic.java, K/io/CompressedOutputStream.java:795-804). */
/* the "skipBlocks" key of the context map (CLI --skip): kz_encode_blocks / kz_compress store a block as a copy block
 * when its first bytes carry the magic number of a compressed format or its order-0 entropy is >= 0.95 * 8 bits
 * (K/io/CompressedOutputStream.java:769-788, Magic.isCompressed, Global.computeFirstOrderEntropy1024). Default off. */
int32_t     kz_ctx_set_skip_blocks(kz_ctx* ctx, int32_t on);
/* the "blockSize" and "entropy" keys of the context map as the TEXT transform reads them: TextCodec sizes its hash map by the
 * stream's block size (K/transform/TextCodec.java:561-575,1068-1081) and TransformFactory picks TextCodec1 or TextCodec2 by the
 * stream's entropy codec (TransformFactory.java:275-286).  kz_encode_blocks / kz_decode_blocks take the entropy codec from
 * their own argument; kz_encode_blocks takes the block size from here AS OF THE CALL (kz_submit_encode_blocks: as of the
 * submit) and refuses a chain with TEXT (-KZ_ERR_MISSING_PARAM) when it was never set, because the decoder is told the block
 * size explicitly and a silent default would write blocks another block size cannot read; kz_decode_blocks takes it from its
 * blockSize argument; kz_transform_forward / _inverse take both from here; kz_compress / kz_decompress set them from the
 * stream.  kz_ctx_set_entropy refuses TPAQX (9): TEXT's extra hash bit under it (TextCodec.java:561-575) is not modelled. */
/* The library's environment switches (KZ_*: diagnostics, A/B runs, the tests' forced schedules -- DESIGN.md 7; none is needed for
 * normal use) are read ONCE, by kz_ctx_create, into the context; no call reads the environment afterwards.  A test or A/B tool
 * that changes the environment of a live context calls this to have it read again.  (No reference counterpart: the reference
 * takes its options through the context map, K/io/CompressedOutputStream.java:140-190.) */
void        kz_ctx_reload_switches(kz_ctx* ctx);
int32_t     kz_ctx_set_block_size(kz_ctx* ctx, int32_t blockSize);
int32_t     kz_ctx_set_entropy(kz_ctx* ctx, uint32_t entropyType);
int32_t     kz_ctx_set_data_type(kz_ctx* ctx, int32_t dataType);
int32_t     kz_ctx_get_data_type(kz_ctx* ctx);
/* every kz_ctx_set_* value back to a fresh context's (checksum none, skipBlocks off, dataType UNDEFINED, block size unset, entropy
 * NONE): the values are sticky like the entries of the reference's context map, and a caller leaving through an error path may not
 * know which ones it had set */
int32_t     kz_ctx_reset(kz_ctx* ctx);
/* One process per GPU, N on one host: pin this process (and the threads it creates later: TEXT / UTF stages, bit assembly,
 * staging copies) to the CPUs of the GPU's NUMA node (/sys/bus/pci/devices/<bdf>/local_cpulist).  Returns the number of CPUs
 * in the new mask, 0 if the topology is not visible (nothing changed), <0 on error.  PROCESS-WIDE: every thread of the process
 * that exists at the time of the call is re-pinned (HIP's helpers, the application's own threads, the workers of contexts bound
 * to other GPUs), so it assumes ONE GPU PER PROCESS; a process that drives several devices must not call it (the last call would
 * move everything to one NUMA node).  The reference has no equivalent: its task pool is one JVM on one socket
 * (K/app/BlockCompressor.java:199-206). */
int32_t     kz_pin_to_device_numa(int32_t deviceId);
/* host CPUs the library's thread pool (TEXT / UTF stages, staging copies, bit assembly) will use: the process's affinity mask cut
 * down to its cgroup CPU quota, if any */
int32_t     kz_host_cpus(void);
/* N processes (one per GPU) under ONE cgroup quota: each takes 1/N of it (rounded up), so that together they stay inside -- a group
 * that runs more busy threads than its quota is frozen as a whole for the rest of every period, GPU-driving threads included.
 * ranksOnHost <= 1 restores the whole quota.  Returns the new kz_host_cpus(). */
int32_t     kz_host_share(int32_t ranksOnHost);
/* HIP stream the context launches on (as void* = hipStream_t) so callers can bracket it with events */
void*       kz_ctx_stream(kz_ctx* ctx);

/* ---- ByteTransform mirror (host buffers; one block) ------------------------------------------ */
/* returns 1 = applied (*produced bytes written), 0 = declined (dst untouched), <0 = error */
int32_t kz_transform_forward(kz_ctx* ctx, uint32_t type, const uint8_t* src, int32_t n,
                             uint8_t* dst, int32_t dstCap, int32_t* produced);
int32_t kz_transform_inverse(kz_ctx* ctx, uint32_t type, const uint8_t* src, int32_t n,
                             uint8_t* dst, int32_t dstCap, int32_t* produced);
int32_t kz_transform_max_encoded_len(uint32_t type, int32_t n);

/* TEXT and UTF (KZ_T_TEXT, KZ_T_UTF) are host stages: the same ByteTransform contract without a context, no GPU touched.
 * entropyType / blockSize = the "entropy" / "blockSize" entries of the reference's context map (TEXT only), *dataType = its
 * "dataType" entry, read and updated (NULL = a transform built without a context). */
int32_t kz_host_stage_forward(uint32_t type, uint32_t entropyType, int32_t blockSize, int32_t* dataType,
                              const uint8_t* src, int32_t n, uint8_t* dst, int32_t dstCap, int32_t* produced);
int32_t kz_host_stage_inverse(uint32_t type, int32_t blockSize, const uint8_t* src, int32_t n,
                              uint8_t* dst, int32_t dstCap, int32_t* produced);

/* ---- EntropyEncoder / EntropyDecoder mirror (host buffers; one block) ------------------------- */
/* returns number of BITS written to out (MSB first, last byte zero padded), <0 = error */
int64_t kz_entropy_encode(kz_ctx* ctx, uint32_t type, const uint8_t* src, int32_t n,
                          uint8_t* out, int64_t outCapBytes);
/* decodes `count` bytes from the bit string in[0..inBits); returns count, or <0; *bitsConsumed set */
int32_t kz_entropy_decode(kz_ctx* ctx, uint32_t type, const uint8_t* in, int64_t inBits,
                          uint8_t* dst, int32_t count, int64_t* bitsConsumed);

/* ---- fused, batched block API ----------------------------------------------------------------- */
typedef struct {
  int64_t bits;                 /* enc: bit length W of the block's private stream */
  int32_t length;               /* enc: postTransformLength ; dec: decoded length */
  int32_t status;               /* 0 ok, else -(K/Error.java code) */
  uint8_t skipFlags;            /* Sequence.getSkipFlags() (K/transform/Sequence.java:243) */
  uint8_t mode;                 /* block mode byte (CompressedOutputStream.java:861-880) */
  uint8_t pad[6];
} kz_block_result;

/*
 * Encode nBlocks independent blocks.  Block b is in[b*inStride .. +lengths[b]); its private stream
 * is written at out[b*outStride ..] (outStride >= kz_max_block_stream_bytes(maxLength)).
 * `lengths` and `results` are host arrays.  memKind says where in/out live (KZ_MEM_HOST: pageable or
 * pinned host memory, copied over PCIe inside the call; KZ_MEM_DEVICE: HBM pointers, no copies).
 * transformType = 8 x 6-bit ids, first transform in the top slot (TransformFactory.java:29-31).
 *
 * Layout contract (maxLength = the largest lengths[b]).  A call outside it returns -KZ_ERR_INVALID_PARAM before anything is
 * copied or launched, `out` and `results` untouched.
 *   in         any address, any inStride >= maxLength (nBlocks > 1), both memory kinds: blocks are read bytewise.  Host memory:
 *              exactly lengths[b] bytes of row b are read.  Device memory: row b may be read up to maxLength bytes whatever
 *              lengths[b] is (chains led by TEXT / UTF copy whole rows back), so in[0 .. (nBlocks-1)*inStride + maxLength) must be
 *              readable; what lies behind lengths[b] never reaches the stream.
 *   out        outStride >= kz_max_block_stream_bytes(maxLength) and a multiple of 4, both memory kinds.  Device memory: `out` itself
 *              4-byte aligned as well (the coders OR 32-bit words into it in place); host memory: any address.
 *   written    nothing outside out[0 .. nBlocks*outStride).  Row b holds the stream in its first (results[b].bits + 7) / 8 bytes,
 *              the spare bits of the last byte zero.  The rest of the row is unspecified: device rows are zeroed and used as
 *              working space, host rows are left as they were behind the stream.
 * nBlocks <= 0 returns 0 and touches nothing.  Batches of more blocks than one launch takes (65 535, or fewer when the scratch
 * arena says so) are coded as consecutive sub-batches; the results are those of the blocks coded one by one.
 */
int32_t kz_encode_blocks(kz_ctx* ctx, uint64_t transformType, uint32_t entropyType,
                         const uint8_t* in, int64_t inStride, const int32_t* lengths, int32_t nBlocks,
                         uint8_t* out, int64_t outStride, kz_block_result* results, int32_t memKind);
/*
 * Decode nBlocks block streams.  Stream b is in[b*inStride ..] with bitLengths[b] bits (W, header
 * included).  Decoded bytes go to out[b*outStride ..] (capacity outStride each, >= blockSize).
 *
 * Layout contract (maxBytes = the largest (bitLengths[b] + 7) / 8).  A call outside it returns -KZ_ERR_INVALID_PARAM before
 * anything is copied or launched, `out` and `results` untouched.
 *   in         any address, both memory kinds: streams are read bytewise or through unaligned loads.  Host memory: inStride >=
 *              maxBytes (nBlocks > 1); exactly (bitLengths[b] + 7) / 8 bytes of slot b are read.  Device memory: inStride >=
 *              maxBytes + KZ_STREAM_SLACK; slot b is read in place, only inside [b*inStride, (b+1)*inStride) and no further than
 *              KZ_STREAM_SLACK bytes behind (bitLengths[b] + 7) / 8 (the decoders load a few bytes ahead of the bit they are at).
 *   no effect  of the spare bits of a stream's last byte, nor of any byte behind it, on status, length or decoded bytes: a block's
 *              result is a function of its bitLengths[b] bits alone (as in the reference, whose bit stream ends there).
 *   out        any address, any outStride >= 0, both memory kinds.  A block that decodes to more than min(outStride, blockSize)
 *              bytes fails with -KZ_ERR_PROCESS_BLOCK.
 *   written    nothing outside out[0 .. nBlocks*outStride); row b holds results[b].length bytes (0 for a failed block), the rest
 *              of the row is unspecified (chains led by TEXT / UTF undo those stages inside the row).
 * nBlocks <= 0 returns 0 and touches nothing.  Larger batches than one launch takes are split like kz_encode_blocks's.
 */
#define KZ_STREAM_SLACK 64
int32_t kz_decode_blocks(kz_ctx* ctx, uint64_t transformType, uint32_t entropyType, int32_t blockSize,
                         const uint8_t* in, int64_t inStride, const int64_t* bitLengths, int32_t nBlocks,
                         uint8_t* out, int64_t outStride, kz_block_result* results, int32_t memKind);
int64_t kz_max_block_stream_bytes(int32_t blockLength);
/*
 * The same two calls queued on the context's worker thread (what SURVEY 8b calls kz_submit / kz_wait): they return a job id
 * (> 0) at once, kz_wait(job) blocks until the call has run and gives its return code, kz_poll(job) says whether it has.  Every
 * array passed (lengths / bitLengths / results, and host in / out buffers) stays the caller's and must stay valid until kz_wait.
 * Jobs of one context run one at a time in submission order; use two contexts to overlap batches (the copies and the encode of
 * batch k+1 under the decode of batch k).  Between a submit and its wait only kz_submit_*, kz_wait and kz_poll may be called on
 * that context.
 */
int64_t kz_submit_encode_blocks(kz_ctx* ctx, uint64_t transformType, uint32_t entropyType,
                                const uint8_t* in, int64_t inStride, const int32_t* lengths, int32_t nBlocks,
                                uint8_t* out, int64_t outStride, kz_block_result* results, int32_t memKind);
int64_t kz_submit_decode_blocks(kz_ctx* ctx, uint64_t transformType, uint32_t entropyType, int32_t blockSize,
                                const uint8_t* in, int64_t inStride, const int64_t* bitLengths, int32_t nBlocks,
                                uint8_t* out, int64_t outStride, kz_block_result* results, int32_t memKind);
/* kz_wait hands a job's return code out ONCE: a second kz_wait / kz_poll on the same id returns -KZ_ERR_INVALID_PARAM. */
int32_t kz_wait(kz_ctx* ctx, int64_t job);
int32_t kz_poll(kz_ctx* ctx, int64_t job);

/* ---- whole .knz stream on host memory (K/io/CompressedOutputStream / CompressedInputStream) --- */
/* returns compressed size in bytes or <0 */
int64_t kz_compress(kz_ctx* ctx, uint64_t transformType, uint32_t entropyType, int32_t blockSize,
                    const uint8_t* src, int64_t n, uint8_t* dst, int64_t dstCap);
int64_t kz_decompress(kz_ctx* ctx, const uint8_t* src, int64_t n, uint8_t* dst, int64_t dstCap);
/* a dstCap that kz_compress never exceeds for n input bytes cut into blockSize blocks (a transform may grow a block:
 * SRT puts up to 1024 bytes of frequencies in front, K/transform/SRT.java MAX_HEADER_SIZE, which is 28 % on 1 KiB
 * blocks of random bytes; the reference's writer simply keeps writing to its OutputStream) */
int64_t kz_compress_bound(int64_t n, int32_t blockSize);
uint64_t kz_transform_type(const int32_t* types, int32_t nb);
/* host-only container helpers (no GPU touched): assemble a .knz from per-block streams gathered in
 * block-id order (stream header :236-313, 5+lw bit length prefix + payload per block :1024-1035, end
 * marker :491-492); index = the serial walk of block prefixes a decoder must do first (:1127-1129). */
/* checksumBits = 0 / 32 / 64: the kz_ctx_set_checksum value the block streams were coded with (it goes into the stream
 * header, :244-250; the block streams already carry their hash bytes) */
int64_t kz_knz_assemble(uint64_t transformType, uint32_t entropyType, int32_t blockSize, int64_t inputSize,
                        int32_t checksumBits, const uint8_t* streams, int64_t stride, const int64_t* bits, int32_t nBlocks,
                        uint8_t* dst, int64_t dstCap);
/* the same, block by block: a gatherer appends block streams in block-id order as they arrive (rank 0 of a multi-GPU job: round
 * r brings blocks r*N .. r*N+N-1 from ranks 0..N-1), holding one round instead of the whole stream.  _open writes the stream header
 * into dst, _add the 5 + lw bit length prefix and the bits of the next block, _close the end marker and returns the size in bytes
 * (or -KZ_ERR_WRITE_FILE when dst was too small); the writer is freed by _close. */
typedef struct kz_knz_writer kz_knz_writer;
kz_knz_writer* kz_knz_writer_open(uint64_t transformType, uint32_t entropyType, int32_t blockSize, int64_t inputSize,
                                  int32_t checksumBits, uint8_t* dst, int64_t dstCap);
int32_t kz_knz_writer_add(kz_knz_writer* w, const uint8_t* stream, int64_t bits);
int64_t kz_knz_writer_close(kz_knz_writer* w);
int32_t kz_knz_index(const uint8_t* src, int64_t n, uint64_t* transformType, uint32_t* entropyType,
                     int32_t* blockSize, int64_t* inputSize, int32_t* checksumBits,
                     int64_t* blockBitOff, int64_t* blockBits, int32_t cap);

/* ---- whole .knz stream on device memory ---------------------------------------------------------
 * The same container as above, written and read with source and destination both in HBM: the stream is byte-identical to
 * kz_compress's, and kz_decompress_device accepts everything kz_decompress accepts.  No payload byte crosses PCIe, except inside
 * kz_encode_blocks / kz_decode_blocks for the blocks their TEXT / UTF host stages take.  What stays on the host: the stream header
 * (at most 26 bytes, one small copy), the bit-offset arithmetic over results[] (5 + lw bit length prefix per block, :1024-1035), and
 * the block-header prechecks (:1025-1095, :1145-1164) on 8 bytes per block that the walk of the length prefixes (:1127-1129, one
 * lane on the device) brings back.
 *
 *   addresses   d_src, d_dst and d_streams may have any address and any alignment; they must not overlap.
 *   read        nothing outside d_src[0 .. n) (kz_knz_assemble_device: of row i only the (bits[i] + 7) / 8 bytes of its stream).  When n
 *               is not a multiple of blockSize, the last, short block is coded in a call of its own with its length as the longest
 *               block (kz_encode_blocks's device contract may read a row up to the call's longest block).
 *   written     nothing outside d_dst[0 .. dstCap).  On success dst[0 .. size) is the stream, the spare bits of its last byte zero;
 *               dst[size .. dstCap) is unspecified; dst need not be zeroed by the caller.  kz_decompress_device: blocks whose whole
 *               blockSize row fits in what is left of dst are decoded straight into it, the others (as a rule the last block of a
 *               destination of the exact size) through staging and a device copy of their bytes; on a fault the blocks in front of
 *               the first failing one are delivered.
 *   returns     kz_compress_device: what kz_compress returns for the same arguments and context settings (checksum, skip blocks,
 *               data type): the size, the first failing block's status, or -KZ_ERR_WRITE_FILE when dstCap is too small;
 *               kz_compress_bound is the bound for both.  kz_decompress_device: what kz_decompress returns for the same bytes and
 *               dstCap, fault or not (a stream is cut at the same block when dst is too small, although the two calls work in
 *               chunks of different sizes).  kz_knz_assemble_device / kz_knz_index_device: as kz_knz_assemble / kz_knz_index
 *               (entries with bits[i] <= 0 are skipped; `bits`, blockBitOff and blockBits are host arrays).
 *   chunks      work proceeds in chunks, one after the other, so staging (the context's grow-only buffers) never exceeds a chunk's rows
 *               whatever n is: kz_compress_device in kz_compress's chunks (about 1 GiB of blocks, 2048 at the most),
 *               kz_decompress_device in kz_decompress's batches (8 GiB of blocks, 2048 at the most: the decoder's serial per-block
 *               chains want many blocks in flight); KZ_STREAM_CHUNK=<blocks> overrides both.  A chunk's first bit is wherever the
 *               previous chunk's last bit ended.
 *   stream      the calls are synchronous and run on the context's stream.
 */
int64_t kz_compress_device(kz_ctx* ctx, uint64_t transformType, uint32_t entropyType, int32_t blockSize,
                           const uint8_t* d_src, int64_t n, uint8_t* d_dst, int64_t dstCap);
int64_t kz_decompress_device(kz_ctx* ctx, const uint8_t* d_src, int64_t n, uint8_t* d_dst, int64_t dstCap);
int64_t kz_knz_assemble_device(kz_ctx* ctx, uint64_t transformType, uint32_t entropyType, int32_t blockSize, int64_t inputSize,
                               int32_t checksumBits, const uint8_t* d_streams, int64_t stride, const int64_t* bits /* host */,
                               int32_t nBlocks, uint8_t* d_dst, int64_t dstCap);
int32_t kz_knz_index_device(kz_ctx* ctx, const uint8_t* d_src, int64_t n, uint64_t* transformType, uint32_t* entropyType,
                            int32_t* blockSize, int64_t* inputSize, int32_t* checksumBits,
                            int64_t* blockBitOff /* host */, int64_t* blockBits /* host */, int32_t cap);

/* ---- many .knz streams on device memory ---------------------------------------------------------
 * kz_compress_device / kz_decompress_device for nStreams buffers in one call: the files of a directory, the tensors of a checkpoint,
 * the pages of a table.  Stream s is the bytes d_src[srcOff[s] .. srcOff[s] + srcLen[s]), its slot d_dst[dstOff[s] .. dstOff[s] +
 * dstCap[s]); offsets are non-negative and relative to the two base pointers (segments in different allocations: pass the lowest
 * address as the base).  The single-stream call is the definition of every result: dstLen[s] is what it returns for segment s and
 * slot s alone under the same context settings, and on success the slot's first dstLen[s] bytes are its bytes.  The serial-per-block
 * kernels take as long for one block as for thousands, so N small buffers cost about one buffer's chain here and N chains in a loop.
 *
 *   addresses   any address and any alignment.  The slots must not overlap each other or any source segment (the caller's duty).
 *   read        nothing outside each stream's own segment: a stream's result depends on its own bytes only, whatever lies between
 *               and behind the segments (every table entry of the kernels carries its own stream's bounds).
 *   written     nothing outside each slot; what lies behind dstLen[s] inside slot s is unspecified, and slots need not be zeroed.
 *   results     kz_compress_many_device: dstLen[s] = the stream's size, the first failing block's status, or -KZ_ERR_WRITE_FILE for
 *               a slot that is too small (kz_compress_many_bound, the sum of kz_compress_bound, suffices for slots laid end to end);
 *               an empty buffer gives the header and end-marker stream.  kz_decompress_many_device: dstLen[s] = the decoded size or
 *               the stream's fault; on a fault the blocks in front of the first failing block are delivered, a short block followed
 *               directly by the next.  Each stream's transform word, entropy id, block size and checksum kind come from its own
 *               header: the streams of one call may differ in all four.  A fault of one stream lives in dstLen[s] only; the other
 *               streams are coded as if it were not there.  kz_last_error: the text of the first failing stream.
 *   returns     0, or a negative code for faults of the call itself: -KZ_ERR_INVALID_PARAM for null pointers with nStreams > 0,
 *               nStreams < 0, or a negative offset, length or capacity; kz_compress_device's block-size code, before anything is
 *               launched; -KZ_ERR_DEVICE.  nStreams == 0 returns 0 and touches nothing.
 *   groups      whole streams are collected into groups of at most one chunk's blocks (kz_compress_device's chunk for the writer,
 *               kz_decompress_device's batch for the reader, KZ_STREAM_CHUNK=<blocks> overrides both).  The blocks of a group are
 *               one batched encode, or one batched decode per distinct header; launches and host waits per group do not grow with
 *               the streams in it.  A stream with more blocks than a group takes goes through the single-stream call on its own.
 *               srcOff, srcLen, dstOff, dstCap and dstLen are host arrays; host memory use is proportional to nStreams and to the
 *               blocks of one group, device staging to one group's rows, neither to the payload.
 *   stream      the calls are synchronous and run on the context's stream.
 */
int64_t kz_compress_many_bound(const int64_t* srcLen, int32_t nStreams, int32_t blockSize);   /* sum of kz_compress_bound(srcLen[s], blockSize) */
int32_t kz_compress_many_device(kz_ctx* ctx, uint64_t transformType, uint32_t entropyType, int32_t blockSize,
                                const uint8_t* d_src, const int64_t* srcOff /* host */, const int64_t* srcLen /* host */, int32_t nStreams,
                                uint8_t* d_dst, const int64_t* dstOff /* host */, const int64_t* dstCap /* host */,
                                int64_t* dstLen /* host, out */);
int32_t kz_decompress_many_device(kz_ctx* ctx,
                                  const uint8_t* d_src, const int64_t* srcOff /* host */, const int64_t* srcLen /* host */, int32_t nStreams,
                                  uint8_t* d_dst, const int64_t* dstOff /* host */, const int64_t* dstCap /* host */,
                                  int64_t* dstLen /* host, out */);

/* ---- seekable .knz streams: a block range, or blocks by an index ----------------------------------
 * Two ways to read part of a stream, each on host memory and on device memory (the _device forms keep kz_decompress_device's
 * memory contract).  Blocks are numbered from 0 in stream order.
 *
 * The RANGE form mirrors the reference reader's context entries "from" / "to" (CompressedInputStream.java:1193-1200, the CLI's
 * --from / --to): from = firstBlock + 1, to = firstBlock + 1 + nBlocks.  It needs no index and walks the length prefixes from the
 * front, so its cost grows with firstBlock (about 2 us per skipped block on the device: the walk is one lane).  Blocks in front of
 * firstBlock are read and skipped as the reference does before it looks at "from" (:1126-1165): length prefix, block-header
 * precheck, staging-row bound, end of stream, in kz_decompress's order; a fault there is returned and nothing is delivered; their
 * payloads are neither unpacked nor decoded, so damage inside them goes unnoticed.  The blocks of the range are decoded and appended
 * to dst from byte 0 exactly as kz_decompress appends (a short block is followed directly by the next; the first failing block
 * ends the call with its status, the blocks of the range in front of it delivered; a block that would start past dstCap gives
 * -KZ_ERR_WRITE_FILE).  At firstBlock + nBlocks the call stops and reads nothing behind the range (the reference still reads that
 * block's bits before it drops it: INTEGRATION 4).  If the end marker comes first, the call returns what it produced, possibly 0.
 *
 * The INDEXED form takes (blockBitOff[i], blockBits[i]) pairs as kz_knz_index / kz_knz_index_device return them: any subset, in any
 * order, with repeats.  Block i is decoded into row dst + i * dstStride; results[i] carries status and length as kz_decode_blocks
 * fills them.  Nothing is walked: its cost does not depend on where the blocks lie in the stream.  The index is the caller's and is
 * not trusted: before anything is unpacked every entry is checked against the stream, each on its own (the kernel k_knz_check on
 * the device): W = blockBits[i] > 0; blockBitOff[i] at least 8 bits behind the stream header; blockBitOff[i] + W <= 8 n; and some
 * lr in 3 .. 34 for which the 5 + lr bits in front of blockBitOff[i] lie behind the stream header and read (lr - 3, W), that is,
 * the walk could have produced the entry at this place.  The check gives memory safety (nothing outside src is read, no row is
 * written past dstStride); it does NOT prove that an entry lies on the true chain of prefixes: bits inside a payload that look like
 * a prefix are accepted, and what follows them is decoded, as a rule into a per-block fault.
 *
 *   addresses   src / d_src and dst / d_dst: any address, any alignment; they must not overlap.  blockBitOff, blockBits and results
 *               are host arrays in all four calls.
 *   read        nothing outside src[0 .. n).
 *   written     range: nothing outside dst[0 .. dstCap); dst[0 .. returned size) is specified, the rest is not.  indexed: nothing
 *               outside dst[0 .. nBlocks * dstStride), and of row i nothing behind its first blockSize bytes; a row holds
 *               results[i].length bytes, the rest of its first blockSize bytes is unspecified (kz_decode_blocks's contract); rows of
 *               entries that were left out of the decode are untouched.
 *   returns     range: bytes produced, or a negative code: the stream header's as from kz_decompress (same kz_last_error texts),
 *               -KZ_ERR_INVALID_PARAM for firstBlock < 0 or nBlocks < 0; nBlocks == 0 returns 0 after the header checks.
 *               indexed: 0, or a negative code for faults of the call: the stream header's, -KZ_ERR_INVALID_PARAM for
 *               dstStride < the stream's block size, for bad arguments, and for the first entry that does not match the stream
 *               (kz_last_error: "index entry %d does not match the stream"; dst untouched), -KZ_ERR_DEVICE.  A fault of one block
 *               (its header precheck, the staging-row bound, its decode) goes to results[i].status; the other entries are decoded.
 *               The transform word, entropy id, block size and checksum kind come from the stream header; the context's checksum
 *               setting is the stream's for the call and restored after it.
 *   chunks      range: kz_decompress_device's chunks from firstBlock on, so a destination that is too small cuts the range where
 *               kz_decompress cuts a stream made of the range's blocks alone.  indexed: chunks of kz_compress_device's size; host
 *               memory proportional to nBlocks (8 bytes per entry) is used besides.  KZ_STREAM_CHUNK=<blocks> overrides both.
 *   stream      the calls are synchronous and run on the context's stream.
 */
int64_t kz_decompress_range(kz_ctx* ctx, const uint8_t* src, int64_t n, int64_t firstBlock, int64_t nBlocks,
                            uint8_t* dst, int64_t dstCap);
int64_t kz_decompress_range_device(kz_ctx* ctx, const uint8_t* d_src, int64_t n, int64_t firstBlock, int64_t nBlocks,
                                   uint8_t* d_dst, int64_t dstCap);
int32_t kz_decode_indexed(kz_ctx* ctx, const uint8_t* src, int64_t n,
                          const int64_t* blockBitOff, const int64_t* blockBits, int32_t nBlocks,
                          uint8_t* dst, int64_t dstStride, kz_block_result* results);
int32_t kz_decode_indexed_device(kz_ctx* ctx, const uint8_t* d_src, int64_t n,
                                 const int64_t* blockBitOff /* host */, const int64_t* blockBits /* host */, int32_t nBlocks,
                                 uint8_t* d_dst, int64_t dstStride, kz_block_result* results /* host */);

/* ---- scan: the blocks of a stream found without the walk, behind damage as well -----------------------
 * Every other way into a stream walks the length prefixes from the front, and one damaged prefix, a lost byte or a cut ends that
 * walk although every block behind the break is intact and independently coded.  The scan asks at EVERY bit position q behind the
 * stream header whether a reader that stands there would accept a block:
 *
 *   accept(q)   the 5 + lr bits at q are a length prefix that fits in the stream, with W > 0, and the block of W bits behind it
 *               (payload at pay = q + 5 + lr) passes what every reader checks before it decodes: the block-header precheck (header
 *               sizes, the checksum byte, which mixes in W), the staging-row bound and pay + W <= 8 n.  succ(q) = pay + W.
 *   final(s)    the prefix at s is the end marker (W == 0) and the byte that holds its last bit is byte n - 1.  An end marker in the
 *               middle of the bytes is no end: runs of zeros are common inside payloads.
 *   path        a sequence of accepted positions, each the succ of the one before.
 *   kept        q is kept if and only if it lies on a path of at least minChain positions, or its path reaches a position s with
 *               final(s).  With a kept q, an accepted succ(q) is kept as well.
 *
 * Between 1.5 (streams of 1 KiB blocks) and 7 (4 MiB blocks) in 10^4 positions of random bytes are accepted, the more the longer a W
 * the stream's block size admits, and almost none of them has an accepted successor: minChain = 4 leaves chance
 * hits of the order of one per hundreds of GiB of incompressible payload, and costs the runs of fewer than 4 intact blocks between
 * two breaks (minChain = 1 keeps every accepted position).  The kept positions come back in ascending q, entry i as
 * prefixBitOff[i] = q, blockBitOff[i] = pay, blockBits[i] = W -- the latter two exactly what kz_knz_index reports for a block and
 * what kz_decode_indexed[_device] takes -- and next[i] = the index of the entry at succ(q), KZ_SCAN_END if final(succ(q)), else
 * KZ_SCAN_BROKEN.  *head = the index of the entry at the first bit behind the stream header, KZ_SCAN_END for a stream that is header
 * plus end marker, else KZ_SCAN_BROKEN.  On an intact stream the chain from *head is kz_knz_index's list.  Only *head says which
 * chain is the stream's own: a .knz stored raw inside a block shows up as a chain of its own, and an accepted position off the
 * stream's chain whose successor is a block of the stream is kept with it (a chance hit inside a payload; or a true prefix read a
 * second time two bits early, with a wider length field and the same W, which gives a second entry with the same blockBitOff and
 * blockBits: DESIGN 7).
 *
 * The device form tests the positions in two passes of the stream (k_knz_scan_count, then k_knz_scan_write: a workgroup per 4 KiB tile and
 * its 16-byte halo, eight positions a lane, the accepted ones gathered in ascending order by per-tile counts and their scan) and
 * links the accepted positions, which are sparse, by binary search (k_knz_scan_link, _run, _mark, _emit).  Its host waits do not
 * grow with n; its scratch (the context's table buffers) is 52 bytes per accepted position and 12 bytes per tile; the link passes'
 * work grows with minChain.
 *
 *   addresses   src / d_src: any address, any alignment.  Every array and every out-pointer is host memory in both calls.  The five
 *               header out-pointers may be NULL; the four arrays may be NULL when cap == 0.
 *   read        nothing outside src[0 .. n); bytes behind n never influence a result.  kz_knz_scan touches no GPU.
 *   written     the header fields; *head; entries [0, min(returned count, cap)) of the four arrays, nothing behind them.  next[]
 *               values point by index whether or not that index is below cap.
 *   returns     the number of kept entries, which may exceed cap (call again with that many), or a negative code: the stream
 *               header's as from kz_knz_index[_device] (n < 20 included; same kz_last_error texts on the device form),
 *               -KZ_ERR_INVALID_PARAM for a null ctx, src, head or array, n < 0, cap < 0 or minChain < 1, -KZ_ERR_DEVICE.
 *   stream      kz_knz_scan_device is synchronous and runs on the context's stream.
 */
enum { KZ_SCAN_END = -1, KZ_SCAN_BROKEN = -2 };
int64_t kz_knz_scan(const uint8_t* src, int64_t n, int32_t minChain,
                    uint64_t* transformType, uint32_t* entropyType, int32_t* blockSize, int64_t* inputSize, int32_t* checksumBits,
                    int64_t* prefixBitOff, int64_t* blockBitOff, int64_t* blockBits, int64_t* next, int64_t cap, int64_t* head);
int64_t kz_knz_scan_device(kz_ctx* ctx, const uint8_t* d_src, int64_t n, int32_t minChain,
                           uint64_t* transformType, uint32_t* entropyType, int32_t* blockSize, int64_t* inputSize, int32_t* checksumBits,
                           int64_t* prefixBitOff /* host */, int64_t* blockBitOff /* host */, int64_t* blockBits /* host */, int64_t* next /* host */,
                           int64_t cap, int64_t* head /* host */);

/* ---- byte-addressed reads: many ranges of the original data in one call ---------------------------
 * "Give me bytes [rangeOff[i], rangeOff[i] + rangeLen[i]) of the original data, for nRanges ranges at once", on host memory and on
 * device memory.  The index (blockBitOff, blockBits, nIndex) is the WHOLE stream's, exactly as kz_knz_index / kz_knz_index_device
 * return it.  Block k holds the original bytes [B[k], B[k + 1]), B = blockByteOff, a table of nIndex + 1 entries.  With blockByteOff
 * == NULL, B[k] = k * blockSize (the stream header's block size): the last index block is the only one that may be short, and its
 * decoded length defines the end of data.  A table says where every block starts, so a stream with short blocks in the middle (what
 * kz_knz_splice[_device] makes of the N streams of a many-stream call, whose input sizes the caller knows) is byte-addressable too;
 * B[nIndex] is then the end of data.
 *
 * Ranges may come in any order, overlap and repeat.  A range is cut at the end of data as a slice is: got[i] is the number of bytes
 * delivered, possibly 0; a range that starts at or behind the end decodes nothing (without a table, a range that starts inside the
 * last block's blockSize bytes has that block decoded to learn where the data ends).  A range's end is never computed: one whose
 * rangeOff + rangeLen leaves int64 reaches the end of data.  The destination is packed by REQUESTED length: range i owns the slot
 * dst[D[i] .. D[i] + rangeLen[i]) with D[i] = the sum of rangeLen[j] for j < i.
 *
 * Each distinct block that some range touches is decoded once, in ascending block order, whatever the order of the ranges; blocks
 * that no range touches are neither decoded nor checked, and their index entries are not looked at.  Only the decoded blocks are
 * verified: block k's decoded length must be B[k + 1] - B[k] (without a table: blockSize for every block but the last), else every
 * range that touches it gets got[i] = -KZ_ERR_INVALID_FILE.  The index is the caller's and is not trusted: every entry the call
 * uses gets the indexed reads' check against the stream (above; k_knz_check on the device) before anything is unpacked.
 *
 *   addresses   src / d_src and dst / d_dst: any address, any alignment; they must not overlap.  blockBitOff, blockBits,
 *               blockByteOff, rangeOff, rangeLen and got are host arrays in both calls.
 *   read        nothing outside src[0 .. n), and of that only the stream header and the blocks that ranges touch.
 *   written     nothing outside dst[0 .. D[nRanges]), and nothing outside the slots at all.  Of slot i the first got[i] bytes are
 *               specified; the rest of a cut range's slot is untouched; the slot of a failed range (got[i] < 0) is unspecified.
 *               got[0 .. nRanges) is written whenever the call returns a size.
 *   returns     D[nRanges], or a negative code for a fault of the call, in this order: -KZ_ERR_INVALID_PARAM for bad arguments
 *               (null pointers, a negative n, nIndex, nRanges, dstCap, rangeOff[i] or rangeLen[i]); the stream header's code as
 *               from kz_decompress; -KZ_ERR_INVALID_PARAM for a table without B[0] == 0 and 1 <= B[k + 1] - B[k] <= blockSize,
 *               before anything but the stream header is read from src; -KZ_ERR_WRITE_FILE for D[nRanges] > dstCap, decided from
 *               the arguments before anything is written; nRanges == 0 returns 0 here, after the header checks;
 *               -KZ_ERR_INVALID_PARAM for the first used entry, in block order, that does not match the stream (kz_last_error:
 *               "index entry %d does not match the stream"; dst untouched); -KZ_ERR_DEVICE.  A block's own fault (its header
 *               precheck, the staging-row bound, its decode, its checksum, its length) goes to got[i] of the ranges that touch
 *               it, as that block's status (of several failing blocks: the first in block order); all other ranges are delivered.
 *               The transform word, entropy id, block size and checksum kind come from the stream header; the context's checksum
 *               setting is the stream's for the call and restored after it.
 *   chunks      the distinct blocks go in chunks of kz_compress_device's size (KZ_STREAM_CHUNK=<blocks> overrides) into the
 *               context's staging rows, blockSize apart.  A segment is one range cut with one block; after each chunk its
 *               segments are copied to their places: memcpy on the host, on the device one k_knz_read launch per 2^20 segments of
 *               the chunk, which spreads the 16-byte destination units of all its segments over the lanes (a 64-byte record
 *               costs 4 or 5 lanes, not a workgroup).  A range that lies across a chunk seam is completed by two launches on the
 *               same stream.  The segment table lives in the context's grow-only table buffers: 32 bytes per segment x the
 *               segments of one launch (32 MiB at the most), pinned and in HBM.  Host memory proportional to the number of
 *               segments of the whole call (about 50 bytes each) and to nRanges is used besides.
 *   cost        a record costs the decode of its whole block, whatever its length: stores of small records choose small blocks.
 *   stream      the calls are synchronous and run on the context's stream.
 */
int64_t kz_read_bytes(kz_ctx* ctx, const uint8_t* src, int64_t n,
                      const int64_t* blockBitOff, const int64_t* blockBits, const int64_t* blockByteOff /* NULL or nIndex + 1 entries */, int32_t nIndex,
                      const int64_t* rangeOff, const int64_t* rangeLen, int32_t nRanges,
                      uint8_t* dst, int64_t dstCap, int64_t* got);
int64_t kz_read_bytes_device(kz_ctx* ctx, const uint8_t* d_src, int64_t n,
                             const int64_t* blockBitOff /* host */, const int64_t* blockBits /* host */, const int64_t* blockByteOff /* host: NULL or nIndex + 1 entries */, int32_t nIndex,
                             const int64_t* rangeOff /* host */, const int64_t* rangeLen /* host */, int32_t nRanges,
                             uint8_t* d_dst, int64_t dstCap, int64_t* got /* host, out */);

/* ---- many-stream index and byte-addressed reads: N streams in one call -----------------------------
 * kz_knz_index_device and kz_read_bytes_device for the N streams that kz_compress_many_device wrote (or any others): a store of
 * compressed objects in HBM is indexed once and then asked for records of several objects at a time.  Streams are described as in
 * kz_decompress_many_device: stream s is d_src[srcOff[s] .. srcOff[s] + srcLen[s]), offsets non-negative and relative to d_src.
 * The single-stream calls define every result.
 *
 * kz_knz_index_many_device: status[s] = the stream's block count or its negative code, the header fields of stream s (written
 * whenever its header parses, as the single call does) and the entries [indexFirst[s], indexFirst[s + 1]) of blockBitOff / blockBits
 * are what kz_knz_index_device gives for segment s alone with a large enough cap.  Bit offsets count from the stream's own first bit.
 * A stream that fails contributes no entries; its fault lives in status[s] only.
 *
 * kz_read_bytes_many_device: range i asks for bytes [rangeOff[i], rangeOff[i] + rangeLen[i]) of the original data of stream
 * rangeStream[i].  Stream s's index is the entries [indexFirst[s], indexFirst[s + 1]) of blockBitOff / blockBits (one
 * kz_knz_index_many_device call gives all three arrays); its table of block starts, if it has one (tableFirst[s] >= 0), is the index
 * length + 1 entries of blockByteOff from tableFirst[s] on and means what it means for kz_read_bytes_device.  The destination is
 * packed by requested length over all ranges in call order: range i owns d_dst[D[i] .. D[i] + rangeLen[i]), D[i] = the sum of
 * rangeLen[j] for j < i.  got[i] and the first got[i] bytes of slot i are what kz_read_bytes_device gives for that stream alone when
 * asked that stream's ranges in their call order: the cut at the end of data, ends past int64, repeats and overlaps, the
 * -KZ_ERR_INVALID_FILE rule on block lengths, and a block's own fault in got[i] of the ranges that touch it.  What is a fault of the
 * whole call in the single-stream form (the stream header's code, a refused table, a first used index entry that does not match the
 * stream) is the fault of that stream alone here: it goes to got[i] of every range of that stream and to streamStatus[s] (0 for
 * every other stream), and every other stream is delivered as if the failing one were not there.
 *
 *   addresses   d_src, d_dst: any address, any alignment; d_dst must not overlap a stream.  All arrays and out-pointers are host memory.
 *   read        nothing outside a stream's own segment (every table entry of the kernels carries its own stream's bounds).  The
 *               index call reads each stream's header and prefixes; the read call only the header and the touched blocks of the
 *               streams that some range names: a stream no range names is not opened at all.
 *   written     the index call: status[0 .. nStreams), indexFirst[0 .. nStreams], the entries below cap.  The read call: nothing
 *               outside the slots; of slot i the first got[i] bytes, the tail of a cut slot is untouched; got[0 .. nRanges) and
 *               streamStatus[0 .. nStreams) (may be NULL) whenever the call returns a size.
 *   returns     kz_knz_index_many_device: the total number of entries, which may exceed cap: indexFirst is complete all the same
 *               and only the entries below cap are written (cap == 0: blockBitOff and blockBits may be NULL); the caller calls
 *               again with that many.  kz_read_bytes_many_device: D[nRanges].  Or a negative code for a fault of the call itself, in
 *               this order: -KZ_ERR_INVALID_PARAM for bad arguments (null pointers with nStreams > 0 resp. nRanges > 0, a negative
 *               count, offset, length or capacity, rangeStream[i] outside [0, nStreams), an indexFirst that descends, a tableFirst[s]
 *               below -1); -KZ_ERR_WRITE_FILE for D[nRanges] > dstCap, decided before anything is written; -KZ_ERR_DEVICE.
 *               nStreams == 0 (index) returns 0 and touches nothing, nRanges == 0 (read) returns 0.  kz_last_error: the text of the
 *               first failing stream in stream order.
 *   chunks      the index call is three launches and three host waits whatever nStreams is: the heads of all streams in one copy
 *               (parsed on the host), a count pass and a fill pass with one lane per stream.  The read call merges the distinct
 *               covering blocks of all named streams into one list ordered by header group (the streams with equal transform word,
 *               entropy id, block size and checksum kind, in order of first appearance), then stream, then block.  Every used entry
 *               is checked against its own stream in launches of 2^18 entries before anything is unpacked.  The list goes in chunks
 *               of kz_compress_device's size for the group's block size (KZ_STREAM_CHUNK=<blocks> overrides), each inside one header
 *               group: one unpack launch, one batched decode under that group's header and checksum kind, and one copy launch per
 *               2^20 segments for the segments of all the chunk's streams.  So N streams of one header cost the launches and waits of
 *               one single-stream call over the same number of blocks.  Tables: 40 bytes per row of a chunk, 56 per checked entry
 *               of a launch, 32 per segment of a launch, pinned and in HBM; host memory proportional to the segments, the rows and
 *               nStreams.
 *   stream      the calls are synchronous and run on the context's stream.
 */
int64_t kz_knz_index_many_device(kz_ctx* ctx, const uint8_t* d_src, const int64_t* srcOff /* host */, const int64_t* srcLen /* host */, int32_t nStreams,
                                 uint64_t* transformType, uint32_t* entropyType, int32_t* blockSize, int64_t* inputSize, int32_t* checksumBits, /* host [nStreams], each may be NULL */
                                 int32_t* status /* host [nStreams] */, int64_t* indexFirst /* host [nStreams + 1] */,
                                 int64_t* blockBitOff /* host */, int64_t* blockBits /* host */, int64_t cap);
int64_t kz_read_bytes_many_device(kz_ctx* ctx, const uint8_t* d_src, const int64_t* srcOff /* host */, const int64_t* srcLen /* host */, int32_t nStreams,
                                  const int64_t* indexFirst /* host [nStreams + 1] */, const int64_t* blockBitOff /* host */, const int64_t* blockBits /* host */,
                                  const int64_t* tableFirst /* host: NULL, or [nStreams] with -1 for a stream without a table */,
                                  const int64_t* blockByteOff /* host: NULL when tableFirst is */,
                                  const int32_t* rangeStream /* host */, const int64_t* rangeOff /* host */, const int64_t* rangeLen /* host */, int32_t nRanges,
                                  uint8_t* d_dst, int64_t dstCap, int64_t* got /* host, out [nRanges] */, int32_t* streamStatus /* host, out [nStreams] or NULL */);

/* ---- byte-addressed writes: many ranges of the original data replaced in one call ------------------
 * "Replace bytes [rangeOff[i], rangeOff[i] + rangeLen[i]) of the original data by these new bytes, for nRanges ranges at once, and
 * give me the new stream", on host memory and on device memory.  The result is a NEW stream in a separate buffer, as with the splice:
 * every block that no range touches is copied bit for bit and not decoded, every touched block is decoded once, patched and encoded
 * once with the chain of the stream's own header.  The index (blockBitOff, blockBits, nIndex) and the table blockByteOff mean what
 * they mean for kz_read_bytes: the index is the WHOLE stream's, block k holds the original bytes [B[k], B[k + 1]), B = blockByteOff
 * or, with NULL, B[k] = k * blockSize with only the last block allowed to be short.
 *
 * The new bytes are packed by length, like the reads' destination: range i brings data[D[i] .. D[i] + rangeLen[i]), D[i] = the sum
 * of rangeLen[j] for j < i, and dataLen must equal D[nRanges].  Ranges may come in any order, overlap and repeat; the result is what
 * applying them one after the other in argument order gives: THE LATER RANGE WINS.  Zero-length ranges are legal and touch nothing.
 * A write never changes the length of the data or the number of blocks: a range must lie wholly inside the data, and no sum may
 * overflow (a range's end is formed only after rangeLen[i] <= end - rangeOff[i] has been seen).  A range that ends behind B[nIndex]
 * (without a table: behind nIndex * blockSize) is refused before anything but the stream header is read; without a table, one that
 * ends behind the real end of a short last block is refused with the same code once that block has been decoded.  Appending stays
 * splice_replace at the block count (kz_knz_splice).
 *
 * A block that some SURVIVING byte touches is "touched" (a range buried whole under later ones touches nothing).  If the surviving
 * new bytes cover all of [B[k], B[k + 1]) and a table gave that length, block k is neither decoded nor checked and its index entry
 * is not looked at: overwriting a damaged block with a table repairs the stream.  Without a table every touched block is decoded
 * (the last one to learn its length).  Every other touched block gets the indexed reads' check of its entry, the block-header
 * precheck, the unpack and the decode exactly as in kz_read_bytes, and its decoded length must be B[k + 1] - B[k].  Untouched blocks
 * are copied verbatim after the splice's check of a piece against its source, which gives memory safety only: a damaged untouched
 * block stays damaged and does not fail the call.
 *
 * Transform word, entropy id, block size and checksum kind come from the stream header; the context's checksum and block-size
 * settings are the stream's for the call and restored after it.  Every chain kz_compress_device takes is taken (TEXT / UTF heads
 * included), and block checksums are computed from the patched bytes.  The result is, byte for byte, kz_knz_assemble of the header's
 * parameters and its own inputSize, the old payload bits of untouched blocks, and what kz_encode_blocks gives for the patched bytes
 * of touched ones.  newBitOff / newBits (both or neither NULL, nIndex entries each) receive the new stream's index: what
 * kz_knz_index of the result returns.  kz_write_bytes_bound returns a dstCap that always suffices: the longest stream header, per
 * block 5 + 34 prefix bits and max(blockBits[k], 8 * kz_max_block_stream_bytes(blockSize)) payload bits, the end marker, in bytes;
 * it uses host arrays only and needs no context.
 *
 *   addresses   src / d_src, data / d_data and dst / d_dst: any address, any alignment; dst overlaps neither of the others.
 *               blockBitOff, blockBits, blockByteOff, rangeOff, rangeLen, newBitOff and newBits are host arrays in both calls.
 *   read        nothing outside src[0 .. n) and data[0 .. dataLen); of src the stream header, the 39 bits in front of every used
 *               entry, the payloads of the decoded blocks and of the kept ones.
 *   written     nothing outside dst[0 .. dstCap).  dst is untouched by every refusal that is decided before the first block is
 *               decoded (arguments, header, table, ranges behind the data, index entries); after that dst[0 .. dstCap) is unspecified
 *               on failure.  On success dst[0 .. size) is the stream, the spare bits of its last byte zero; dst[size .. dstCap) is
 *               untouched by the host form and unspecified for the device form.  dst need not be zeroed.
 *   returns     the new stream's size, or a negative code.  The call is all or nothing; there is no per-range status.  In this
 *               order: -KZ_ERR_INVALID_PARAM for bad arguments (null pointers, negative sizes, dataLen != D[nRanges], only one of
 *               newBitOff / newBits); the stream header's code as from kz_decompress; -KZ_ERR_INVALID_PARAM for a bad table and for
 *               a range behind the data (kz_last_error: "range %d ends behind the data"); -KZ_ERR_INVALID_PARAM for the first used
 *               index entry, in block order, that does not match the stream ("index entry %d does not match the stream"); a
 *               touched block's own fault (precheck, staging bound, decode, checksum, length) as that block's code, of several
 *               failing blocks the first in block order ("block %d: ..."); -KZ_ERR_WRITE_FILE when the stream outgrows dstCap,
 *               decided from the bit arithmetic before the chunk that would cross it is written; -KZ_ERR_DEVICE.  nRanges == 0, or a
 *               call in which no byte survives, returns a bit-exact copy of the stream (header, all blocks, end marker) for a
 *               stream whose header is the one this library writes for its parameters.
 *   chunks      the touched blocks go in ascending order in chunks of kz_compress_device's size (KZ_STREAM_CHUNK=<blocks>
 *               overrides) through staging rows blockSize apart: unpack and decode, the patch (memcpy on the host; on the device
 *               k_knz_write, one launch per 2^20 segments, which spreads the 16-byte units of the ROW side of all its segments over
 *               the lanes: a 64-byte record costs 4 or 5 lanes, not a workgroup), one batched encode, then one copy in k_knz_splice's
 *               manner of every kept block since the previous chunk's last touched block and of the chunk's recoded blocks, in
 *               launches of at most one chunk's pieces; a chunk's first bit is wherever the previous one's last bit ended.  After
 *               the last chunk come the kept tail and the end marker.  Segments are disjoint, so no order between lanes, launches
 *               or segments decides anything.  Tables live in the context's grow-only buffers (32 bytes per segment of one launch,
 *               48 per piece of one launch); row staging is bounded by one chunk.  Host memory proportional to nRanges (about 60
 *               bytes per range and per segment) and to the touched blocks (8 bytes each) is used besides.
 *   cost        the touched blocks' decode and encode, and a bit copy of the rest; nothing that is decoded grows with the
 *               untouched blocks.
 *   stream      the calls are synchronous and run on the context's stream.
 */
int64_t kz_write_bytes_bound(const int64_t* blockBits, int32_t nIndex, int32_t blockSize);
int64_t kz_write_bytes(kz_ctx* ctx, const uint8_t* src, int64_t n,
                       const int64_t* blockBitOff, const int64_t* blockBits, const int64_t* blockByteOff /* NULL or nIndex + 1 entries */, int32_t nIndex,
                       const int64_t* rangeOff, const int64_t* rangeLen, int32_t nRanges,
                       const uint8_t* data, int64_t dataLen,
                       uint8_t* dst, int64_t dstCap, int64_t* newBitOff, int64_t* newBits /* nIndex entries each, both or neither NULL */);
int64_t kz_write_bytes_device(kz_ctx* ctx, const uint8_t* d_src, int64_t n,
                              const int64_t* blockBitOff /* host */, const int64_t* blockBits /* host */, const int64_t* blockByteOff /* host: NULL or nIndex + 1 entries */, int32_t nIndex,
                              const int64_t* rangeOff /* host */, const int64_t* rangeLen /* host */, int32_t nRanges,
                              const uint8_t* d_data, int64_t dataLen,
                              uint8_t* d_dst, int64_t dstCap, int64_t* newBitOff /* host, out */, int64_t* newBits /* host, out */);

/* ---- many-stream byte-addressed writes: ranges of N streams in one call ----------------------------
 * kz_write_bytes_device for records of several of the N streams of a store at a time: the counterpart of kz_read_bytes_many_device.
 * Streams, indices and tables are described exactly as there; slots exactly as for kz_compress_many_device: the new stream s goes to
 * d_dst[dstOff[s] .. dstOff[s] + dstCap[s]).  Slots overlap neither each other, nor any source segment, nor d_data: that is the
 * caller's duty.  The new bytes are packed over ALL ranges in call order: range i brings d_data[D[i] .. D[i] + rangeLen[i]), D[i] = the
 * sum of rangeLen[j] for j < i, and dataLen must equal D[nRanges].
 *
 * The single-stream call defines every result.  A stream is NAMED if at least one range names it (a zero-length range counts).  For a
 * named stream s take what kz_write_bytes_device returns and writes when called on that stream alone with that stream's ranges in
 * their call order, its own slot and dstCap[s]: dstLen[s] is that return value, the first dstLen[s] bytes of slot s are those bytes,
 * and the entries [indexFirst[s], indexFirst[s + 1]) of newBitOff / newBits are that call's new index.  So the later range wins,
 * ranges buried whole under later ones touch nothing, a wholly covered block with a table is neither decoded nor checked, block
 * lengths are checked, and a copy of the stream results when no byte survives.  A stream no range names is not opened: its dstLen[s]
 * is 0, its slot and its new* entries are untouched.
 *
 * A fault stays with its stream.  What fails the whole single-stream call (the header's code, a refused table, "range %d ends behind
 * the data", "index entry %d does not match the stream", a touched block's own fault, -KZ_ERR_WRITE_FILE for a stream that outgrows
 * its slot) goes to dstLen[s] of that stream alone here, and every other stream comes out byte for byte as if the failing one were not
 * in the call.  The range number in a text is the range's number in the call.  Of a stream with several faults the one this call
 * meets first is reported: a block's fault before the room of the chunk it is in.
 *
 * kz_write_bytes_many_bound needs no context: slotCap[s] (may be NULL) = kz_write_bytes_bound of stream s's entries and blockSize[s];
 * it returns their sum, or -KZ_ERR_INVALID_PARAM.
 *
 *   addresses   d_src, d_data, d_dst: any address, any alignment.  All arrays and out-pointers are host memory.
 *   read        nothing outside a named stream's own segment and d_data[0 .. dataLen); of a stream what the single call reads.
 *   written     nothing outside the slots of the named streams.  A failed stream's slot is unspecified inside its own bounds; a slot
 *               behind its dstLen[s] bytes likewise.  dstLen[0 .. nStreams) whenever the arguments pass.
 *   returns     0, or a negative code for a fault of the call itself, decided before anything is read from the device:
 *               -KZ_ERR_INVALID_PARAM for bad arguments (null pointers with a positive count, a negative count, offset, length or
 *               capacity, rangeStream[i] outside [0, nStreams), an indexFirst that descends, a tableFirst[s] below -1, dataLen !=
 *               D[nRanges], only one of newBitOff / newBits); -KZ_ERR_DEVICE.  nRanges == 0 returns 0, sets every dstLen[s] to 0 and
 *               touches nothing else.  kz_last_error: the text of the first failing stream in stream order.
 *   chunks      the touched blocks of all named streams, covered ones included, form one list ordered by header group (equal
 *               transform word, entropy id, block size and checksum kind, in order of first appearance), then stream, then block,
 *               cut into chunks of kz_compress_device's size for the group's block size (KZ_STREAM_CHUNK=<blocks> overrides), each
 *               inside one group.  Every used entry, the kept blocks' and the decoded ones', is checked against its own stream in
 *               launches of 2^18 entries before anything is unpacked.  Per chunk: one unpack launch and one batched decode, the
 *               patch (k_knz_write, one launch per 2^20 segments of all the chunk's streams), one batched encode (the rows of a
 *               stream that failed in the chunk are left out, which may split it), and the emit: k_knz_splice_many, one launch per
 *               chunk's size of pieces, writes for every stream with rows in the chunk its kept blocks since its last emission and
 *               its recoded ones behind its own last bit, the stream header with its first emission, the kept tail and the end
 *               marker with its last.  A named stream with no touched block is a whole copy in the first emit launch with room.
 *               So N streams of one header cost the launches and host waits of one single-stream call over as many blocks.
 *               Device staging is bounded by one chunk; tables: 40 bytes per row, 32 per segment of a launch, 72 per span and 48
 *               per piece of an emit launch, pinned and in HBM.  Host memory proportional to the ranges, the segments, the touched
 *               blocks and nStreams.
 *   cost        the touched blocks' decode and encode and a bit copy of the rest of the named streams.
 *   stream      the call is synchronous and runs on the context's stream.
 */
int64_t kz_write_bytes_many_bound(const int64_t* indexFirst /* [nStreams + 1] */, const int64_t* blockBits, const int32_t* blockSize /* [nStreams] */, int32_t nStreams,
                                  int64_t* slotCap /* out [nStreams], may be NULL */);
int32_t kz_write_bytes_many_device(kz_ctx* ctx, const uint8_t* d_src, const int64_t* srcOff /* host */, const int64_t* srcLen /* host */, int32_t nStreams,
                                   const int64_t* indexFirst /* host [nStreams + 1] */, const int64_t* blockBitOff /* host */, const int64_t* blockBits /* host */,
                                   const int64_t* tableFirst /* host: NULL, or [nStreams] with -1 for a stream without a table */,
                                   const int64_t* blockByteOff /* host: NULL when tableFirst is */,
                                   const int32_t* rangeStream /* host */, const int64_t* rangeOff /* host */, const int64_t* rangeLen /* host */, int32_t nRanges,
                                   const uint8_t* d_data, int64_t dataLen,
                                   uint8_t* d_dst, const int64_t* dstOff /* host */, const int64_t* dstCap /* host */, int64_t* dstLen /* host, out [nStreams] */,
                                   int64_t* newBitOff /* host, out */, int64_t* newBits /* host, out: laid out by indexFirst, both or neither NULL */);

/* ---- splice: a new .knz stream out of blocks of existing ones, without recoding -------------------
 * Blocks are independent of one another, and a stream is its header, then per block 5 + lw prefix bits and W payload bits, then the
 * end marker (:1024-1035, :483-493): a stream made of blocks taken from existing streams is a bit-granular copy.  One call joins the
 * streams kz_compress_many_device (or N ranks) wrote, cuts a block range out as a stream of its own, or replaces or appends a block
 * after only the new bytes were compressed.  No block is decoded.
 *
 * Source s is the .knz stream src[srcOff[s] .. srcOff[s] + srcLen[s]) (offsets relative to one base pointer, as in the many-stream
 * calls).  Piece i is the block of source pieceSrc[i] whose payload is pieceBits[i] bits at bit pieceBitOff[i], counted from that
 * source's first bit, exactly as kz_knz_index / kz_knz_index_device return it: any subset, in any order, with repeats, from any mix
 * of sources.  The result is the stream header, each piece as a minimal-width prefix and its payload bits verbatim, the end
 * marker, the spare bits of the last byte zero: byte for byte kz_knz_assemble(the sources' header parameters, the pieces' extracted
 * bit strings, their W).  The transform word, entropy id, block size and checksum kind come from the sources' own headers, which
 * must agree in all four (a source that no piece names is parsed and compared all the same); inputSize is the caller's, with the
 * meaning kz_knz_assemble gives it (0: unknown).  nSrc >= 1; nPieces == 0 gives the header and end-marker stream.
 * kz_knz_splice_bound returns a dstCap that suffices: the longest stream header, 5 + lw + W bits per piece, the end marker, in bytes.
 *
 * Nothing is trusted: before a bit is copied every piece is checked against ITS OWN source with the rule of the indexed reads
 * (above; k_knz_check_many on the device), using that source's header end and length.  As there, the check gives memory safety and
 * does not prove that a piece lies on the true chain of prefixes.
 *
 *   addresses   src / d_src and dst / d_dst: any address, any alignment; dst overlaps no source.  srcOff, srcLen, pieceSrc,
 *               pieceBitOff and pieceBits are host arrays in both forms.  kz_knz_splice works on host memory and needs no context
 *               and no GPU, like kz_knz_assemble.
 *   read        nothing outside a source's own segment, not even a neighbour's bytes in the same buffer.
 *   written     nothing outside dst[0 .. dstCap).  On success dst[0 .. size) is the stream, dst[size .. dstCap) is untouched by the
 *               host form and unspecified for the device form; dst need not be zeroed.  On every refusal except -KZ_ERR_DEVICE
 *               dst is untouched.
 *   returns     the stream's size, or in this order: -KZ_ERR_INVALID_PARAM for bad arguments (null pointers, nSrc < 1, nPieces < 0,
 *               a negative offset, length, inputSize or dstCap) or a pieceSrc[i] outside 0 .. nSrc; the first bad source header's
 *               code as the reader of a stream header gives it, on the source's first min(26, srcLen[s]) bytes (kz_last_error:
 *               "source %d: ..."); -KZ_ERR_INVALID_PARAM for sources that disagree
 *               ("source %d differs from source 0 in ...") and for the first piece that fails its check ("piece %d does not match
 *               its source"); -KZ_ERR_WRITE_FILE when dstCap is too small, decided from the bit arithmetic before anything is
 *               written; -KZ_ERR_DEVICE (device form).  The host form has no context and returns the code alone.
 *   chunks      the device form takes the pieces in chunks of kz_compress_device's size (KZ_STREAM_CHUNK=<blocks> overrides): per
 *               chunk one launch checks the pieces and one copies them, whatever the chunk holds; a chunk's first bit is wherever
 *               the previous chunk's last bit ended.  Payload bits go from the sources straight to their place in dst (k_knz_splice:
 *               any byte misalignment, any of the 8 x 8 bit phases of the two sides); there are no staging rows.  Tables live in
 *               the context's grow-only buffers; host memory proportional to nSrc and nPieces (8 bytes each) is used besides.
 *   stream      the device call is synchronous and runs on the context's stream.
 */
int64_t kz_knz_splice_bound(const int64_t* pieceBits, int32_t nPieces);
int64_t kz_knz_splice(const uint8_t* src, const int64_t* srcOff, const int64_t* srcLen, int32_t nSrc,
                      const int32_t* pieceSrc, const int64_t* pieceBitOff, const int64_t* pieceBits, int32_t nPieces,
                      int64_t inputSize, uint8_t* dst, int64_t dstCap);
int64_t kz_knz_splice_device(kz_ctx* ctx, const uint8_t* d_src, const int64_t* srcOff /* host */, const int64_t* srcLen /* host */, int32_t nSrc,
                             const int32_t* pieceSrc /* host */, const int64_t* pieceBitOff /* host */, const int64_t* pieceBits /* host */, int32_t nPieces,
                             int64_t inputSize, uint8_t* d_dst, int64_t dstCap);

/* ---- instrumentation (bench.py / roofline) ----------------------------------------------------- */
/* blocks that went through a TEXT / UTF stage on a HOST thread since the last reset (process-wide counter; inverse = 0: forward,
 * 1: inverse).  The stage timers KZ_STAGE_HOST_FWD / _INV measure the TEXT / UTF stage's wall time INCLUDING its device forms
 * (kz_text_fwd_gpu.hip: the TEXT forward of TextCodec2 and TextCodec1 streams, kz_utf_fwd_gpu.hip, kz_text_gpu.hip): this counter says
 * how much of the stage the host really did. */
int64_t kz_host_stage_blocks(int32_t inverse, int32_t reset);
void    kz_set_timing(kz_ctx* ctx, int32_t enable);     /* hipEvent-bracket every stage of the next calls */
int32_t kz_get_stage_count(kz_ctx* ctx);
float   kz_get_stage_ms(kz_ctx* ctx, int32_t stage);    /* accumulated since last kz_reset_timing */
int64_t kz_get_stage_alg_bytes(kz_ctx* ctx, int32_t stage);
void    kz_reset_timing(kz_ctx* ctx);
/* per-kernel: HIP events recorded on the context's stream around every kernel launch */
void        kz_set_kernel_timing(kz_ctx* ctx, int32_t enable);
int32_t     kz_get_kernel_count(void);
const char* kz_get_kernel_name(int32_t id);
double      kz_get_kernel_ms(kz_ctx* ctx, int32_t id);        /* summed launch durations since reset */
double      kz_get_kernel_max_ms(kz_ctx* ctx, int32_t id);    /* longest single launch since reset (launches on the decoder's side streams overlap) */
int64_t     kz_get_kernel_launches(kz_ctx* ctx, int32_t id);
void        kz_reset_kernel_timing(kz_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif
