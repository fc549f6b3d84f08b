"""Helpers of the RLE Lossless tests: the plain numpy restatement of the `mmnn_rle_expand` contract (include/mmnn_sts.h), a builder of
fragments from hand-made segment streams, the shapes and the hostile streams that the CPU and GPU tests share, and the payload as ingest
stages it (the fixture of the stand-alone host check is tests/_dicom_stream_harness.py).  Shares no code with mmnn_sts_amd (neither the
kernel's core nor synth_dicom's encoder)."""
import struct

import numpy as np

from tests._dicom_stream_harness import align16


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def packbits_decode(segment, n):
    """The first `n` bytes that the PackBits stream `segment` expands to, and whether it fell short.  A control byte c < 128 copies the
    next c + 1 bytes, c > 128 repeats the next byte 257 - c times, 128 does nothing.  Decoding stops once n bytes are out: the run that
    overfills is clipped and the rest of the stream is ignored.  A run whose bytes do not all lie inside the stream gives nothing and ends
    it; a stream that ends early leaves the rest of the plane zero.  Returns (uint8 array of n bytes, 0 or 1)."""
    segment = bytes(segment)
    out = bytearray()
    p = 0
    while len(out) < n and p < len(segment):
        c = segment[p]
        if c == 128:
            p += 1
        elif c < 128:
            if p + 1 + c + 1 > len(segment):
                break
            out += segment[p + 1:p + 2 + c]
            p += c + 2
        else:
            if p + 2 > len(segment):
                break
            out += bytes([segment[p + 1]]) * (257 - c)
            p += 2
    short = int(len(out) < n)
    out = out[:n] + bytes(n - min(n, len(out)))
    return np.frombuffer(bytes(out), dtype=np.uint8), short


def rle_expand_ref(fragments, segments, x, y, bits):
    """`fragments`: per frame its bytes; `segments`: per frame the (B, 2) table of (offset into the fragment, length), B = bits / 8,
    clamped into the fragment as the kernel clamps.  Returns (pixels: (z, y, x) little-endian unsigned words of `bits` bits, status: (z,)
    int32).  Segment s is byte B - 1 - s of the word."""
    B = bits // 8
    pixels = np.zeros((len(fragments), y * x, B), dtype=np.uint8)
    status = np.zeros(len(fragments), dtype=np.int32)
    for k, (fragment, table) in enumerate(zip(fragments, segments)):
        fragment = bytes(fragment)
        for s in range(B):
            off = min(max(int(table[s][0]), 0), len(fragment))
            length = min(max(int(table[s][1]), 0), len(fragment) - off)
            plane, short = packbits_decode(fragment[off:off + length], x * y)
            pixels[k, :, B - 1 - s] = plane
            status[k] |= short
    return pixels.reshape(len(fragments), y, x, B).view(f"<u{B}").reshape(len(fragments), y, x), status


def rle_fragment(planes_as_streams):
    """A fragment from arbitrary segment streams (the most significant byte plane first): the 64-byte header, then the streams as they
    are -- no padding, no check, so a test can build what no encoder would.  Returns (bytes, (B, 2) table of offset and length)."""
    offsets, at = [], 64
    for stream in planes_as_streams:
        offsets.append(at)
        at += len(stream)
    header = struct.pack("<16I", len(planes_as_streams), *offsets, *([0] * (15 - len(offsets))))
    return header + b"".join(bytes(s) for s in planes_as_streams), np.array([[o, len(s)] for o, s in zip(offsets, planes_as_streams)], dtype=np.int64)


def literal(data):
    """`data` as literal runs of at most 128 bytes."""
    data = bytes(data)
    return b"".join(bytes([len(data[i:i + 128]) - 1]) + data[i:i + 128] for i in range(0, len(data), 128))


def repeat(value, n):
    """n >= 2 copies of `value` as repeat runs of at most 128 (a single byte left over as a literal of one)."""
    out = b""
    while n >= 2:
        take = min(n, 128)
        out += bytes([257 - take, value])
        n -= take
    return out + (bytes([0, value]) if n else b"")


def segment_table(fragment, bits):
    """The (B, 2) table a fragment's own header describes (what dicom.read_file derives)."""
    count, *offsets = struct.unpack_from("<16I", fragment, 0)
    used = offsets[:bits // 8]
    return np.array([[a, b - a] for a, b in zip(used, used[1:] + [len(fragment)])], dtype=np.int64)


# ---- the cases the CPU round trip, the host check and the GPU tests share ------------------------------------------------------------
def _noise(rng, shape, dtype):
    """Words whose every byte plane has no two equal neighbours along a row: an encoder finds no repeat run in them."""
    info = np.iinfo(dtype)
    a = rng.integers(info.min, int(info.max) + 1, shape, dtype=np.int64).astype(dtype)
    planes = a.view(np.uint8).reshape(shape + (a.dtype.itemsize,))
    for i in range(1, shape[0]):
        same = planes[i] == planes[i - 1]
        planes[i][same] += 1
    return a


def volumes():
    """{name: (x, y, z) integer volume}: the shapes of the issue, the smallest at which each path can go wrong."""
    rng = np.random.default_rng(2024)
    v = {"4x3x1_u8": rng.integers(0, 4, (4, 3, 1)).astype("u1"), "5x3x2_i16": rng.integers(-3, 3, (5, 3, 2)).astype("i2"),
         "130x2x2_constant_rows": np.broadcast_to(np.array([[1, 11], [2, 12]], dtype="u1"), (130, 2, 2)).copy(),
         "257x1x1_noise": _noise(rng, (257, 1, 1), "u1")}
    a = rng.integers(-70000, 70000, (64, 64, 3)).astype("i4")
    a[:, :, 1] = -77                            # one constant slice: its segments are a few dozen bytes, the others' kilobytes
    a[:32, :, 2] = 5
    v["64x64x3_i32"] = a
    v["256x64x2_i16_noise"] = _noise(rng, (256, 64, 2), "i2")
    return v


def hand_streams(chunk):
    """{name: (x, y, bits, [streams of frame 0], ...)}: well-formed streams no encoder of rows would write, for a kernel that passes a
    segment through LDS `chunk` bytes at a time.  A window starts at the 16-byte boundary at or in front of the segment's first byte;
    the stream here is the first segment of a fragment on a 16-byte boundary and starts at its byte 64, so it crosses the chunk
    boundaries at stream bytes chunk, 2 * chunk, ..."""
    rng = np.random.default_rng(7)
    edge = chunk
    cases = {}
    for name, straddler, produced in (("literal", lambda: literal(rng.integers(0, 256, 100, dtype=np.uint8).tobytes()), 100), ("repeat", lambda: repeat(201, 77), 77),
                                      ("noops", lambda: bytes([128]) * 300, 0)):
        for back in ((1, 50) if name == "literal" else (1,) if name == "repeat" else (1, 150)):
            # filler of literal-of-one runs (2 stream bytes each) up to `back` bytes in front of the boundary, the straddler, a tail, twice
            # (the second boundary is met at another phase of the stream)
            stream, count = b"", 0
            for boundary in (edge, edge + chunk):
                fill = (boundary - back - len(stream)) // 2
                stream += b"".join(bytes([0, v]) for v in rng.integers(0, 256, fill, dtype=np.uint8))
                if (boundary - back - len(stream)) % 2:
                    stream += bytes([128])
                assert len(stream) == boundary - back
                stream += straddler() + repeat(9, 3)
                count += fill + produced + 3
            cases[f"{name}_straddles_{back}_before"] = (count, 1, 8, [stream])
    n = 70 * 61
    cases["one_byte_literals"] = (70, 61, 8, [b"".join(bytes([0, v]) for v in rng.integers(0, 256, n, dtype=np.uint8))])       # x*y runs: the run-count bound
    cases["runs_cross_row_ends"] = (10, 7, 16, [repeat(3, 33) + literal(bytes(range(30))) + repeat(250, 7), literal(bytes(range(64))) + repeat(1, 6)])
    cases["last_run_overfills"] = (9, 5, 8, [literal(bytes(range(40))) + repeat(77, 128)])
    cases["literal_overfills"] = (9, 5, 8, [repeat(7, 30) + literal(bytes(range(100, 200)))])
    cases["junk_behind_a_full_plane"] = (6, 4, 8, [repeat(5, 24) + bytes([127, 1, 2, 3, 255, 128, 130])])
    big = chunk * 2 + 77                        # more output than one window of input yields at once, from long repeats
    cases["long_repeats"] = (big, 3, 8, [repeat(11, big) + repeat(12, big) + repeat(13, big)])
    return cases


def malformed_streams():
    """{name: stream}: each is a plane of an 8 x 6 frame (48 bytes) that falls short."""
    return {"cut_mid_literal": repeat(4, 20) + bytes([9, 1, 2, 3, 4]), "cut_after_repeat_control": literal(bytes(range(10))) + bytes([200]),
            "noops_only": bytes([128]) * 37, "zero_length": b"", "ends_between_runs": repeat(8, 47)}


MALFORMED_PRODUCED = {"cut_mid_literal": 20, "cut_after_repeat_control": 10, "noops_only": 0, "zero_length": 0, "ends_between_runs": 47}      # bytes out before the plane falls short


def malformed_frames(name, bits=8):
    """(fragments, tables, x, y, bits): the malformed stream as a plane of frame 1 of 3; frames 0 and 2 are sound and differ."""
    x, y = 8, 6
    B = bits // 8
    rng = np.random.default_rng(11)
    sound = lambda: [literal(rng.integers(0, 256, x * y, dtype=np.uint8).tobytes()) for _ in range(B)]
    bad = sound()
    bad[B - 1] = malformed_streams()[name]
    pairs = [rle_fragment(s) for s in (sound(), bad, sound())]
    return [p[0] for p in pairs], [p[1] for p in pairs], x, y, bits


# ---- the payload as ingest stages it; a record of the host check's fixture (tests/_dicom_stream_harness.py) is one int64 ---------------
RECORD = np.dtype("<i8")


def pack_payload(fragments, tables):
    """(payload with every fragment on a 16-byte boundary, (z, B, 2) table of payload offsets and lengths), as ingest stages them."""
    payload, table = bytearray(), []
    for fragment, t in zip(fragments, tables):
        t = np.array(t, dtype=np.int64)
        t[:, 0] += align16(payload)
        table.append(t)
        payload += fragment
    return bytes(payload), np.stack(table)
