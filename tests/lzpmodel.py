"""CPU model of LZP, the LZ predictor transform, written from the reference's Java (K/transform/LZCodec.java, class LZPCodec,
:973-1287), not from the HIP kernels.  Line numbers cite that file.  Bitstream 7 only: minMatch is 64 in both directions.

forward(data, dst_len=None, stats=None) -> (ok, out)
inverse(data, dst_len, stats=None) -> (ok, out)

`ok` is the method's return value, `out` the bytes up to `output.index` (empty where the method returns before it moves the
index).  `dst_len` is the room in the output slice (forward, :1034; default: getMaxEncodedLength) and `output.length` with
`output.index` 0 (inverse, :1158, :1163).  Where the Java would throw (an array index outside the array) the block has failed:
(False, b""), as in rltmodel.py.

`stats`, when given, is a dict whose counters are incremented:
  matches          matches coded (forward) / decoded (inverse)
  chained          matches whose length took at least one 0xFE byte
  overlapping      inverse: matches copied byte by byte (:1232-1235: source and destination overlap)
  fc_escaped       0xFC literals followed by 0xFF (ref != 0)
  fc_plain         0xFC literals with ref == 0 (no escape)
  fc_escaped_near  the same two, at one of the first three positions after a match (ctx mixes both byte orders there)
  fc_plain_near
"""
HASH_SEED = 0x7FEB352D                                           # :974
HASH_SHIFT = 16                                                  # :975-976
MIN_MATCH = 64                                                   # :978
MIN_BLOCK_LENGTH = 128                                           # :979
MATCH_FLAG = 0xFC                                                # :980
M32 = 0xFFFFFFFF

STAT_KEYS = ("matches", "chained", "overlapping", "fc_escaped", "fc_plain", "fc_escaped_near", "fc_plain_near")


def new_stats():
    return dict.fromkeys(STAT_KEYS, 0)


def max_encoded_length(n):                                       # :1284-1286
    return n + 16 if n <= 1024 else n + n // 64


def _find_match(src, src_idx, ref, max_match):                   # :1257-1273
    best = 0
    while best + 8 <= max_match:
        a = src[src_idx + best:src_idx + best + 8]
        if a != src[ref + best:ref + best + 8]:
            b = src[ref + best:ref + best + 8]
            k = 0
            while a[k] == b[k]:
                k += 1
            return best + k
        best += 8
    return best


def forward(data, dst_len=None, stats=None):
    count = len(data)
    if count == 0:                                               # :1024-1025
        return True, b""
    if dst_len is None:
        dst_len = max_encoded_length(count)
    if dst_len < max_encoded_length(count):                      # :1034-1035
        return False, b""
    if count < MIN_BLOCK_LENGTH:                                 # :1038-1039
        return False, b""
    st = stats if stats is not None else new_stats()
    src = bytes(data)
    hashes = [0] * 65536                                         # :1041-1046
    src_end = count
    dst_end = count - (count >> 6)                               # :1053
    dst = bytearray(src[0:4])                                    # :1057-1060 (len(dst) is dstIdx)
    ctx = int.from_bytes(src[0:4], "little")                     # :1061
    src_idx = 4
    near = 0                                                     # positions left of the three that follow a match
    while src_idx < src_end - MIN_MATCH and len(dst) < dst_end:  # :1066
        h = ((HASH_SEED * ctx) & M32) >> HASH_SHIFT
        ref = hashes[h]
        hashes[h] = src_idx
        best = 0
        if ref != 0 and src[ref + 60:ref + 64] == src[src_idx + 60:src_idx + 64]:   # :1073-1076
            best = _find_match(src, src_idx, ref, src_end - src_idx)
        if best < MIN_MATCH:                                     # :1079-1092
            val = src[src_idx]
            ctx = ((ctx << 8) | val) & M32
            dst.append(val)
            src_idx += 1
            if val == MATCH_FLAG:
                key = "fc_escaped" if ref != 0 else "fc_plain"
                st[key] += 1
                if near:
                    st[key + "_near"] += 1
                if ref != 0:
                    if len(dst) >= dst_end:
                        return False, bytes(dst)
                    dst.append(0xFF)
            if near:
                near -= 1
            continue
        src_idx += best                                          # :1094-1111
        ctx = int.from_bytes(src[src_idx - 4:src_idx], "little")
        dst.append(MATCH_FLAG)
        st["matches"] += 1
        near = 3
        best -= MIN_MATCH
        if best >= 254:
            st["chained"] += 1
        while best >= 254:
            best -= 254
            dst.append(0xFE)
            if len(dst) >= dst_end:
                break
        if len(dst) >= dst_end:
            return False, bytes(dst)
        dst.append(best)
    while src_idx < src_end and len(dst) < dst_end:              # :1114-1128
        h = ((HASH_SEED * ctx) & M32) >> HASH_SHIFT
        ref = hashes[h]
        hashes[h] = src_idx
        val = src[src_idx]
        ctx = ((ctx << 8) | val) & M32
        dst.append(val)
        src_idx += 1
        if val == MATCH_FLAG:
            key = "fc_escaped" if ref != 0 else "fc_plain"
            st[key] += 1
            if near:
                st[key + "_near"] += 1
            if ref != 0:
                if len(dst) >= dst_end:
                    return False, bytes(dst)
                dst.append(0xFF)
        if near:
            near -= 1
    return (src_idx == count and len(dst) < dst_end), bytes(dst)  # :1132


def inverse(data, dst_len, stats=None):
    count = len(data)
    if count == 0:                                               # :1146-1147
        return True, b""
    if dst_len < count:                                          # :1163-1164
        return False, b""
    if count < 4:                                                # :1173-1176 read src[0..3]: with a slice of exactly `count` bytes
        return False, b""                                        # that throws, and with a longer array srcIdx = 4 > srcEnd fails :1243
    st = stats if stats is not None else new_stats()
    src = bytes(data)
    src_end = count
    dst_end = dst_len
    hashes = [0] * 65536
    dst = bytearray(src[0:4])                                    # dst_len >= count >= 4
    ctx = int.from_bytes(dst[0:4], "little")                     # :1177
    src_idx = 4
    while src_idx < src_end:                                     # :1181
        h = ((HASH_SEED * ctx) & M32) >> HASH_SHIFT
        ref = hashes[h]
        hashes[h] = len(dst)
        val = src[src_idx]
        if ref == 0 or val != MATCH_FLAG:                        # :1186-1195
            if len(dst) >= dst_end:
                return False, bytes(dst)
            dst.append(val)
            ctx = ((ctx << 8) | val) & M32
            src_idx += 1
            if val == MATCH_FLAG:
                st["fc_plain"] += 1
            continue
        src_idx += 1
        if src_idx >= src_end:                                   # :1199-1200
            return False, bytes(dst)
        if src[src_idx] == 0xFF:                                 # :1202-1211
            if len(dst) >= dst_end:
                return False, bytes(dst)
            dst.append(MATCH_FLAG)
            ctx = ((ctx << 8) | MATCH_FLAG) & M32
            src_idx += 1
            st["fc_escaped"] += 1
            continue
        m_len = MIN_MATCH                                        # :1213-1225 (a Python int: no wrap)
        if src[src_idx] == 0xFE:
            st["chained"] += 1
            while src_idx < src_end and src[src_idx] == 0xFE:
                src_idx += 1
                m_len += 254
            if src_idx >= src_end:
                return False, bytes(dst)
        m_len += src[src_idx]
        src_idx += 1
        dst_idx = len(dst)
        if dst_idx + m_len > dst_end:                            # :1227-1228
            return False, bytes(dst)
        st["matches"] += 1
        if ref + m_len < dst_idx:                                # :1230-1235
            dst += dst[ref:ref + m_len]
        else:
            st["overlapping"] += 1
            dist = dst_idx - ref
            seg = bytes(dst[ref:dst_idx])
            dst += (seg * (m_len // dist + 1))[:m_len]
        ctx = int.from_bytes(dst[-4:], "little")                 # :1238
    return src_idx == src_end, bytes(dst)                        # :1243
