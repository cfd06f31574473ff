"""CPU model of RLT, the escaped run-length transform, written from the reference's Java (K/transform/RLT.java), not from the HIP
kernels.  Line numbers cite that file.

forward(data, dst_len, entropy, data_type, have_ctx=True) -> (ok, out, data_type_out)
inverse(data, dst_len) -> (ok, out)

`dst_len` is `dst.length`, the length of the output ARRAY (:115, :320), which the reference uses as its bound whatever the slice
says; the slices start at index 0 here.  `ok` is the method's return value, `out` the bytes up to `output.index`.  `have_ctx=False`
is `new RLT()` (:46-49): no context, so the best escape is searched and no type is stored back.  Where the Java would throw,
katmodels.JavaException is raised."""
from katmodels import JavaException, detect_simple_type

RUN_LEN_ENCODE1 = 224                                            # :32
RUN_LEN_ENCODE2 = (255 - RUN_LEN_ENCODE1) << 8                    # :33   7 936
RUN_THRESHOLD = 3                                                # :35
MAX_RUN = 0xFFFF + RUN_LEN_ENCODE2 + RUN_THRESHOLD - 1            # :36   73 473
MAX_RUN4 = MAX_RUN - 4                                           # :37   73 469
DEFAULT_ESCAPE = 0xFB                                            # :38


def max_encoded_length(n):
    return n + 32 if n <= 512 else n                             # :419-421


def _emit_run_length(dst, dst_idx, run):                         # :276-292
    run -= RUN_THRESHOLD
    if run >= RUN_LEN_ENCODE1:
        if run < RUN_LEN_ENCODE2:
            run -= RUN_LEN_ENCODE1
            dst[dst_idx] = RUN_LEN_ENCODE1 + (run >> 8)
            dst_idx += 1
        else:
            run -= RUN_LEN_ENCODE2
            dst[dst_idx] = 0xFF
            dst[dst_idx + 1] = (run >> 8) & 0xFF
            dst_idx += 2
    dst[dst_idx] = run & 0xFF
    return dst_idx + 1


def forward(data, dst_len, entropy="NONE", data_type="UNDEFINED", have_ctx=True):
    try:
        return _forward(data, dst_len, entropy, data_type, have_ctx)
    except IndexError as e:                                      # a Java array index outside the array
        raise JavaException("ArrayIndexOutOfBoundsException: %s" % e)


def inverse(data, dst_len):
    try:
        return _inverse(data, dst_len)
    except IndexError as e:
        raise JavaException("ArrayIndexOutOfBoundsException: %s" % e)


def _forward(data, dst_len, entropy, data_type, have_ctx):
    count = len(data)
    if count == 0:                                               # :70-71
        return True, b"", data_type
    if count < 16:                                               # :78-79
        return False, b"", data_type
    if dst_len < max_encoded_length(count):                      # :86-87 (output.length is the array's here)
        return False, b"", data_type
    src = bytearray(data)
    dst = bytearray(dst_len)
    dt = "UNDEFINED"
    find_best_escape = True
    if have_ctx:                                                 # :94-108
        dt = data_type
        if dt in ("DNA", "BASE64", "UTF8"):
            return False, b"", data_type
        if entropy.upper() in ("NONE", "ANS0", "HUFFMAN", "RANGE"):
            find_best_escape = False
    escape = DEFAULT_ESCAPE                                      # :110-115
    src_idx = 0
    dst_idx = 0
    src_end = count
    src_end4 = src_end - 4
    dst_end = dst_len
    if find_best_escape:                                         # :117-149
        freqs = [0] * 256
        for b in data:
            freqs[b] += 1
        if dt == "UNDEFINED":
            dt = detect_simple_type(count, freqs)
            if have_ctx and dt != "UNDEFINED":
                data_type = dt
            if dt in ("DNA", "BASE64", "UTF8"):
                return False, b"", data_type
        min_idx = 0
        if freqs[min_idx] > 0:
            for i in range(1, 256):
                if freqs[i] < freqs[min_idx]:
                    min_idx = i
                    if freqs[i] == 0:
                        break
        escape = min_idx
    res = True                                                   # :151-158
    run = 0
    prev = src[src_idx]
    src_idx += 1
    dst[dst_idx] = escape
    dst[dst_idx + 1] = prev
    dst_idx += 2
    if prev == escape:
        dst[dst_idx] = 0
        dst_idx += 1
    while True:                                                  # :161-224
        if prev == src[src_idx]:
            src_idx += 1
            run += 1
            if prev == src[src_idx]:
                src_idx += 1
                run += 1
                if prev == src[src_idx]:
                    src_idx += 1
                    run += 1
                    if prev == src[src_idx]:
                        src_idx += 1
                        run += 1
                        if run < MAX_RUN4 and src_idx < src_end4:
                            continue
        if run > RUN_THRESHOLD:                                  # :185-197
            if dst_idx + 6 >= dst_end:
                res = False
                break
            dst[dst_idx] = prev
            dst_idx += 1
            if prev == escape:
                dst[dst_idx] = 0
                dst_idx += 1
            dst[dst_idx] = escape
            dst_idx += 1
            dst_idx = _emit_run_length(dst, dst_idx, run)
        elif prev != escape:                                     # :198-205
            if dst_idx + run >= dst_end:
                res = False
                break
            while run > 0:
                dst[dst_idx] = prev
                dst_idx += 1
                run -= 1
        else:                                                    # :206-216
            if dst_idx + 2 * run >= dst_end:
                res = False
                break
            while run > 0:
                dst[dst_idx] = escape
                dst[dst_idx + 1] = 0
                dst_idx += 2
                run -= 1
        prev = src[src_idx]                                      # :218-223
        src_idx += 1
        run = 1
        if src_idx >= src_end4:
            break
    if res:                                                      # :226-260
        if prev != escape:
            if dst_idx + run < dst_end:
                while run > 0:
                    dst[dst_idx] = prev
                    dst_idx += 1
                    run -= 1
        else:
            if dst_idx + 2 * run < dst_end:
                while run > 0:
                    dst[dst_idx] = escape
                    dst[dst_idx + 1] = 0
                    dst_idx += 2
                    run -= 1
        while src_idx < src_end and dst_idx < dst_end:           # :243-257
            if src[src_idx] == escape:
                if dst_idx + 2 >= dst_end:
                    res = False
                    break
                dst[dst_idx] = escape
                dst[dst_idx + 1] = 0
                dst_idx += 2
                src_idx += 1
                continue
            dst[dst_idx] = src[src_idx]
            dst_idx += 1
            src_idx += 1
        res = res and (src_idx == src_end)                       # :259
    res = res and (dst_idx < src_idx)                            # :262
    return res, bytes(dst[:dst_idx]), data_type


def _inverse(data, dst_len):
    count = len(data)
    if count == 0:                                               # :303-304
        return True, b""
    src = bytearray(data)
    dst = bytearray(dst_len)
    src_idx = 0
    dst_idx = 0
    src_end = count
    dst_end = dst_len
    res = True
    escape = src[src_idx]                                        # :322
    src_idx += 1
    if src[src_idx] == escape:                                   # :324-333 (a one-byte input reads src[1]: throws)
        src_idx += 1
        if src_idx < src_end and src[src_idx] != 0:
            return False, b""
        dst[dst_idx] = escape
        dst_idx += 1
        src_idx += 1
    while src_idx < src_end:                                     # :336-404
        if src[src_idx] != escape:
            if dst_idx >= dst_end:
                break
            dst[dst_idx] = src[src_idx]
            dst_idx += 1
            src_idx += 1
            continue
        src_idx += 1
        if src_idx >= src_end:                                   # :348-351
            res = False
            break
        if dst_idx == 0:
            raise IndexError("dst[-1]")
        val = dst[dst_idx - 1]                                   # :353
        run = src[src_idx]
        src_idx += 1
        if run == 0:                                             # :356-363
            if dst_idx >= dst_end:
                break
            dst[dst_idx] = escape
            dst_idx += 1
            continue
        if run == 0xFF:                                          # :366-374
            if src_idx >= src_end - 1:
                res = False
                break
            run = (src[src_idx] << 8) | src[src_idx + 1]
            src_idx += 2
            run += RUN_LEN_ENCODE2
        elif run >= RUN_LEN_ENCODE1:                             # :375-383
            if src_idx >= src_end:
                res = False
                break
            run = ((run - RUN_LEN_ENCODE1) << 8) | src[src_idx]
            src_idx += 1
            run += RUN_LEN_ENCODE1
        run += RUN_THRESHOLD - 1                                 # :385
        if dst_idx + run > dst_end or run > MAX_RUN:             # :387-390
            res = False
            break
        dst[dst_idx:dst_idx + run] = bytes([val]) * run          # :393-403
        dst_idx += run
    res = res and (src_idx == src_end)                           # :406
    return res, bytes(dst[:dst_idx])
