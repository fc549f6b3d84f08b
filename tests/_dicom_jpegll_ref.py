"""Helpers of the JPEG Lossless tests: the plain restatement of the `mmnn_jpegll_decode` contract (include/mmnn_sts.h) -- byte stuffing,
the canonical codes of T.81 Annex C decoded bit by bit as Annex F.2.2.3 does, the differences of H.1.2.2 and predictor 1 walked serially
--, an encoder of its own that writes one bit at a time, the volumes, hand-made streams and hostile streams that the CPU and GPU tests
share, and the payload as ingest stages it (the fixture of the stand-alone host check is tests/_dicom_stream_harness.py).  Shares no
code with mmnn_sts_amd (neither the kernel's core nor synth_dicom's encoder)."""
import struct

import numpy as np

from tests._dicom_stream_harness import align16

K3 = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))                 # T.81 Table K.3
EXTENDED = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0), tuple(range(17)))           # one more code per length up to 14 bits
RECORD = np.dtype([("offset", "<i8"), ("length", "<i8"), ("precision", "<i4"), ("bits", "u1", 16), ("huffval", "u1", 17), ("reserved", "u1", 3)])


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def code_table(bits, huffval):
    """[(length, code, value)] in code order, as Annex C generates them: HUFFSIZE from BITS, then HUFFCODE counting up and shifting
    left at every change of size.  Values BITS counts but HUFFVAL does not hold are 0."""
    sizes = [l for l, n in enumerate(bits, 1) for _ in range(int(n))]
    out, code, at = [], 0, sizes[0] if sizes else 0
    for k, size in enumerate(sizes):
        code <<= size - at
        at = size
        out.append((size, code, int(huffval[k]) if k < len(huffval) else 0))
        code += 1
    return out


def unstuff(data):
    """The entropy-coded bytes of `data` as bits: FF 00 is the byte FF; FF followed by anything else, or FF as the last byte, ends the
    data there."""
    data, out, i = bytes(data), bytearray(), 0
    while i < len(data):
        if data[i] == 0xFF:
            if i + 1 < len(data) and data[i + 1] == 0:
                out.append(0xFF)
                i += 2
                continue
            break
        out.append(data[i])
        i += 1
    return "".join(f"{b:08b}" for b in out)


def decode_differences(data, bits, huffval, n):
    """(the first differences of the stream modulo 2^16, at most n; 1 when a symbol was cut before n were out, else 0)."""
    stream, table = unstuff(data), {(l, c): v for l, c, v in code_table(bits, huffval)}
    out, p = [], 0
    while len(out) < n:
        peek = (stream[p:p + 16] + "1" * 16)[:16]             # padded with 1-bits behind the end
        ssss = next((table[(l, int(peek[:l], 2))] for l in range(1, 17) if (l, int(peek[:l], 2)) in table), None)
        if ssss is None or ssss > 16:
            return out, 1
        length = next(l for l in range(1, 17) if (l, int(peek[:l], 2)) in table)
        extra = ssss if ssss < 16 else 0
        if p + length + extra > len(stream):
            return out, 1
        if ssss == 0:
            d = 0
        elif ssss == 16:
            d = 32768
        else:
            v = int(stream[p + length:p + length + extra], 2)
            d = v if v >= 1 << (ssss - 1) else v - (1 << ssss) + 1
        out.append(d & 0xFFFF)
        p += length + extra
    return out, 0


def decode_frame(data, bits, huffval, precision, x, y, bits_allocated):
    """((y, x) unsigned words of `bits_allocated` bits, status): the differences of the stream, the missing ones 0, walked under
    predictor 1 modulo 2^16; the word is the low bits_allocated bits."""
    diffs, status = decode_differences(data, bits, huffval, x * y)
    diffs = diffs + [0] * (x * y - len(diffs))
    out = np.zeros((y, x), dtype=np.int64)
    for j in range(y):
        for i in range(x):
            predicted = 1 << (precision - 1) if i == 0 and j == 0 else out[j - 1, 0] if i == 0 else out[j, i - 1]
            out[j, i] = (int(predicted) + diffs[j * x + i]) & 0xFFFF
    return (out & ((1 << bits_allocated) - 1)).astype(f"<u{bits_allocated // 8}"), status


def decode_ref(payload, records, x, y, bits_allocated):
    """`records`: a RECORD array over `payload`.  Offset and length are clamped into the payload and the precision into 2..16, as the
    kernel clamps.  Returns (pixels (z, y, x), status (z,) int32)."""
    payload = bytes(payload)
    pixels, status = [], []
    for r in records:
        off = min(max(int(r["offset"]), 0), len(payload))
        length = min(max(int(r["length"]), 0), len(payload) - off)
        words, bad = decode_frame(payload[off:off + length], r["bits"].tolist(), r["huffval"].tolist(), min(max(int(r["precision"]), 2), 16), x, y, bits_allocated)
        pixels.append(words)
        status.append(bad)
    return np.stack(pixels), np.array(status, dtype=np.int32)


# ---- an encoder of its own ---------------------------------------------------------------------------------------------------------------
def symbol_bits(table, d):
    """The bits of one difference d (-32767..32768) under `table` = (BITS, HUFFVAL)."""
    codes = {v: (l, c) for l, c, v in code_table(*table)}
    ssss = 0 if d == 0 else 16 if d == 32768 else abs(d).bit_length()
    length, code = codes[ssss]
    bits = f"{code:0{length}b}"
    if 1 <= ssss <= 15:
        bits += f"{d if d > 0 else d + (1 << ssss) - 1:0{ssss}b}"
    return bits


def pack_bits(bits):
    """A bit string as entropy-coded bytes: the last byte padded with 1-bits, a zero byte stuffed behind every FF."""
    bits += "1" * (-len(bits) % 8)
    raw = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))
    return raw.replace(b"\xff", b"\xff\x00")


def differences_of(frame, precision):
    """The differences (-32767..32768) of a (y, x) frame of unsigned words under predictor 1, walked sample by sample."""
    frame = np.asarray(frame).astype(np.int64)
    out = []
    for j in range(frame.shape[0]):
        for i in range(frame.shape[1]):
            predicted = 1 << (precision - 1) if i == 0 and j == 0 else frame[j - 1, 0] if i == 0 else frame[j, i - 1]
            d = (int(frame[j, i]) - int(predicted)) & 0xFFFF
            out.append(d - 65536 if d > 32768 else d)
    return out


def samples_of(diffs, precision):
    """The samples (modulo 2^16) of one row that `diffs` produce from 2^(P-1) on."""
    return ((1 << (precision - 1)) + np.cumsum(np.asarray(diffs, dtype=np.int64))) & 0xFFFF


def encode(frame, precision, table=EXTENDED):
    return pack_bits("".join(symbol_bits(table, d) for d in differences_of(frame, precision)))


def record(offset, length, precision, table):
    r = np.zeros((), dtype=RECORD)
    r["offset"], r["length"], r["precision"] = offset, length, precision
    r["bits"] = table[0]
    r["huffval"][:len(table[1])] = table[1]
    return r


def pack_payload(streams):
    """`streams`: per frame (data, precision, table).  (payload with every frame's data on a 16-byte boundary behind 16 bytes of other
    content, RECORD array), as ingest stages the fragments."""
    payload, records = bytearray(), []
    for data, precision, table in streams:
        align16(payload)
        payload += b"\xff\xd8" + bytes(14)      # (a fragment starts with markers, never with data)
        records.append(record(len(payload), len(data), precision, table))
        payload += bytes(data)
    return bytes(payload), np.array(records, dtype=RECORD)


def scan_of(fragment):
    """(offset of the data behind SOS, precision, (BITS, HUFFVAL) of table 0) of a JPEG stream with one DHT table, walked marker by marker."""
    fragment = bytes(fragment)
    assert fragment[:2] == b"\xff\xd8"
    at, precision, table = 2, None, None
    while True:
        marker, n = fragment[at + 1], struct.unpack_from(">H", fragment, at + 2)[0]
        body = fragment[at + 4:at + 2 + n]
        if marker == 0xC4:
            count = sum(body[1:17])
            table = (tuple(body[1:17]), tuple(body[17:17 + count]))
        if marker == 0xC3:
            precision = body[0]
        at += 2 + n
        if marker == 0xDA:
            return at, precision, table


def pack_fragments(fragments):
    """(payload with every fragment on a 16-byte boundary, RECORD array): whole JPEG streams as ingest stages them, each record
    pointing behind its stream's SOS and reaching to the fragment's end."""
    payload, records = bytearray(), []
    for fragment in fragments:
        at, precision, table = scan_of(fragment)
        records.append(record(align16(payload) + at, len(fragment) - at, precision, table))
        payload += bytes(fragment)
    return bytes(payload), np.array(records, dtype=RECORD)


# ---- the cases the CPU round trip, the host check and the GPU tests share ------------------------------------------------------------
def precision_of(vol, bits_stored):
    return bits_stored if bits_stored is not None else vol.dtype.itemsize * 8


def volumes():
    """{name: ((x, y, z) integer volume, bits_stored or None)}: u1, i2 and u2 at P 8, 12 and 16; the shapes 1x1, 1x7, 7x1, 5x7, 33x17 and
    64x64; constant, ramp, noise and steps of +-32768."""
    rng = np.random.default_rng(2025)
    v = {"1x1x2_u1": (rng.integers(0, 256, (1, 1, 2)).astype("u1"), None), "1x7x1_i2_p16": (rng.integers(-32768, 32768, (1, 7, 1)).astype("i2"), None),
         "7x1x2_u2_p12": (rng.integers(0, 4096, (7, 1, 2)).astype("u2"), 12), "5x7x3_u2_constant": (np.full((5, 7, 3), 40000, "u2"), None)}
    ramp = (np.arange(33)[:, None, None] * 3 + np.arange(17)[None, :, None] * 100 + np.arange(2)[None, None, :]).astype("i2") - 900
    v["33x17x2_i2_ramp"] = (ramp, None)
    steps = np.zeros((33, 17, 1), dtype="u2")
    steps[::2] = 32768                          # every difference along a row is 32768 (SSSS 16)
    steps[:, ::3] += 7
    v["33x17x1_u2_steps_of_32768"] = (steps, None)
    v["64x64x2_i2_noise"] = (rng.integers(-32768, 32768, (64, 64, 2)).astype("i2"), None)
    v["64x64x1_u1_noise"] = (rng.integers(0, 256, (64, 64, 1)).astype("u1"), None)
    v["33x17x2_u2_p12_noise"] = (rng.integers(0, 4096, (33, 17, 2)).astype("u2"), 12)
    return v


ONE_BIT = ((1,) + (0,) * 15, (0,))                                          # SSSS 0 is the code 0
SIXTEEN_BIT = ((1,) + (0,) * 14 + (1,), (0, 15))                            # SSSS 15 is the code 1000000000000000


def _row_case(diffs, precision=16, table=EXTENDED, trailer=b"\xff\xd9"):
    """One frame of one row from its differences: (x, y, bits_allocated, [(data, precision, table)])."""
    samples = samples_of(diffs, precision)
    assert differences_of(samples[None, :], precision) == [int(d) for d in diffs]
    return (len(diffs), 1, 16, [(pack_bits("".join(symbol_bits(table, int(d)) for d in diffs)) + trailer, precision, table)])


def hand_streams(chunk):
    """{name: (x, y, bits_allocated, [(data, precision, table) per frame])}: well-formed streams at the edges of a kernel that passes
    the data through LDS `chunk` raw bytes at a time.  `pack_payload` puts every frame's data on a 16-byte boundary, so the data
    crosses the chunk edges at its own bytes chunk, 2 * chunk, ..."""
    rng = np.random.default_rng(7)
    cases = {}
    n = 8 * chunk + 3                           # every symbol one bit long: the most rounds of pointer doubling
    cases["one_bit_symbols"] = (n, 1, 8, [(pack_bits("0" * n) + b"\xff\xd9", 8, ONE_BIT)])
    flips = [20000 + int(v) for v in rng.integers(0, 9000, 3 * 200)]           # every symbol 16 + 15 bits long, three rows of 200
    diffs = [d if k % 2 == 0 else -d for k, d in enumerate(flips)]
    frame = np.zeros((3, 200), dtype=np.int64)
    at = 1 << 15
    for j in range(3):
        for i in range(200):
            at = ((frame[j - 1, 0] if i == 0 and j else at) + diffs[j * 200 + i]) & 0xFFFF
            frame[j, i] = at
    data = encode(frame, 16, SIXTEEN_BIT)
    assert len(data) > 2 * chunk and all(abs(d).bit_length() == 15 for d in differences_of(frame, 16))
    cases["31_bit_symbols"] = (200, 3, 16, [(data + b"\xff\xd9", 16, SIXTEEN_BIT)])
    # a symbol that starts at bit `o` of the chunk's last byte and straddles the edge; where a code of 8 - o bits exists (o <= 5) the
    # code ends at the edge and the extra bits lie behind it.  In front of it: two-bit symbols (difference 0), and one of five bits where
    # the start is odd.  Negative differences: their extra bits start with 0, so no FF arises and raw and unstuffed positions agree.
    width = {l: v for l, _, v in code_table(*EXTENDED)}                         # code length -> SSSS
    for o in range(8):
        start = 8 * chunk - 8 + o
        ssss = width[8 - o] if o <= 5 else 5
        lead = [0] * ((start - (5 if start % 2 else 0)) // 2) + ([-2] if start % 2 else [])
        diffs = lead + [-(1 << (ssss - 1)) - 1] + [3, -1, 0, 200, -7]
        case = _row_case(diffs)
        assert sum(len(symbol_bits(EXTENDED, d)) for d in lead) == start and 0xFF not in case[3][0][0][:-2]       # (all but the EOI)
        cases[f"straddles_the_edge_from_bit_{o}"] = case
    # FF as the last raw byte of a chunk, its stuffed 00 the first of the next: the 14-bit code of SSSS 16 from bit 8 (chunk - 1) - 2 on
    case = _row_case([0] * ((8 * (chunk - 1) - 2) // 2) + [32768] + [0] * 10)
    assert case[3][0][0][chunk - 2:chunk + 2] == b"\x03\xff\x00\xe0"
    cases["ff_ends_a_chunk"] = case
    case = _row_case([0] * (4 * chunk))         # the frame is full at the chunk's last bit; EOI follows
    assert case[3][0][0] == bytes(chunk) + b"\xff\xd9"
    cases["full_at_a_chunk_edge"] = case
    cases["trailing_garbage"] = _row_case([5, -300, 32768, 0, 1, -1], trailer=b"\x12\xff\x00\x34\xff\xd9\xff\xff\x00\x99" + bytes(range(200, 256)))
    frames = [rng.integers(1, 2048, (7, 5)) for _ in range(3)]                  # z = 3, three tables (K.3 has no category 12)
    own = ((0, 0, 3, 3, 3, 3, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0), (12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0))
    cases["three_tables"] = (5, 7, 16, [(encode(f, 12, t) + b"\xff\xd9", 12, t) for f, t in zip(frames, (K3, EXTENDED, own))])
    cases["one_sample"] = (1, 1, 16, [(encode(np.array([[1234]]), 16) + b"\xff\xd9", 16, EXTENDED)])
    return cases


def malformed_streams():
    """{name: (data, table)}: each the data of an 8 x 6 frame at P = 8 (48 samples, the values of `_sound(1)`) that falls short."""
    whole = encode(_sound(1), 8)
    diffs = differences_of(_sound(1), 8)
    bits = [symbol_bits(EXTENDED, d) for d in diffs]
    stream = "".join(bits)
    starts = np.concatenate(([0], np.cumsum([len(b) for b in bits])))
    codes = [len(b) - (abs(d).bit_length() if d else 0) for b, d in zip(bits, diffs)]
    # the byte boundaries (the data is whole bytes) that fall inside a code, inside extra bits and between two symbols
    mid_code = next(e for k in range(10, 48) for e in range(int(starts[k]) + 1, int(starts[k]) + codes[k]) if e % 8 == 0)
    mid_extra = next(e for k in range(10, 48) for e in range(int(starts[k]) + codes[k], int(starts[k + 1])) if e % 8 == 0 and e > starts[k] + codes[k])
    between = next(int(e) for e in starts[10:48] if e % 8 == 0)
    k = 20
    poisoned = (EXTENDED[0], tuple(17 if v == abs(diffs[k]).bit_length() else v for v in EXTENDED[1]))
    return {"ends_mid_code": (_bytes_of(stream[:mid_code]), EXTENDED), "ends_mid_extra_bits": (_bytes_of(stream[:mid_extra]), EXTENDED),
            "ends_between_symbols": (_bytes_of(stream[:between]), EXTENDED),
            "marker_inside": (whole[:len(whole) // 2] + b"\xff\xd0" + whole[len(whole) // 2:], EXTENDED),
            "all_ones_prefix": (pack_bits("".join(bits[:k]) + "1" * 40), EXTENDED),
            "table_entry_17": (whole, poisoned), "no_data": (b"", EXTENDED)}


def _bytes_of(bits):
    """A bit string of whole bytes as entropy-coded bytes (a zero stuffed behind every FF), with no padding."""
    assert len(bits) % 8 == 0
    return bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8)).replace(b"\xff", b"\xff\x00")


def _sound(k):
    return np.random.default_rng([11, k]).integers(0, 256, (6, 8))


def malformed_frames(name, bits_allocated=8):
    """(streams for `pack_payload`, x, y, bits_allocated): the malformed data as frame 1 of 3; frames 0 and 2 are sound and differ."""
    data, table = malformed_streams()[name]
    sound = lambda k: (encode(_sound(k), 8) + b"\xff\xd9", 8, EXTENDED)
    return [sound(0), (data, 8, table), sound(2)], 8, 6, bits_allocated


def lying_records():
    """{name: (streams, patch)}: sound frames whose record of frame 1 is patched by `patch(records, payload)` to lie about where its
    data is.  Every lie leaves frame 1 short."""
    streams = malformed_frames("no_data")[0]
    streams[1] = (encode(_sound(1), 8) + b"\xff\xd9", 8, EXTENDED)

    def lie(offset=None, length=None):
        def patch(records, payload):
            if offset is not None:
                records[1]["offset"] = offset(records, payload) if callable(offset) else offset
            if length is not None:
                records[1]["length"] = length
        return patch

    return {"negative_offset": (streams, lie(-300, 200)), "offset_far_past_the_payload": (streams, lie(1 << 40, 50)),
            "negative_length": (streams, lie(None, -5)), "offset_at_the_last_byte": (streams, lie(lambda r, p: len(p) - 1, 99)),
            "runs_into_the_next_frame": (streams, lie(lambda r, p: int(r[1]["offset"]) + int(r[1]["length"]) - 5, 1 << 40)),
            "length_past_the_payload_from_the_markers": (streams, lie(lambda r, p: int(r[1]["offset"]) - 16, 1 << 40))}
