"""What the RLE Lossless and the JPEG Lossless tests share around their own streams and restatements: the bytes of encapsulated
PixelData items, the 16-byte packing of a payload, the binary fixture and the build-and-run of a stand-alone host check
(tests/stream_check.hpp), the table of calls that `mmnn_rle_expand` / `mmnn_jpegll_decode` refuse before any launch, the call of either
with every buffer inside a patterned guard buffer, and the comparison with a restatement.  A plain module: each test file keeps its
own fixtures, cases and tests."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
GUARD = 256
PATTERN = 0xA5


# ---- bytes ---------------------------------------------------------------------------------------------------------------------------
def write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


def item(value, tag=(0xFFFE, 0xE000), length=None):
    return struct.pack("<HHI", tag[0], tag[1], len(value) if length is None else length) + value


DELIMITER = item(b"", (0xFFFE, 0xE0DD))


def align16(payload):
    """Pad the bytearray `payload` with zeros to a 16-byte boundary, where ingest puts the next fragment; returns that offset."""
    payload += bytes(-len(payload) % 16)
    return len(payload)


# ---- the stand-alone host check of a core ----------------------------------------------------------------------------------------------
def write_fixture(path, cases, record):
    """`cases`: [(x, y, z, bits_allocated, payload, table)].  Little endian: int32 count; per case int32 x, y, z, bits_allocated, int64
    payload_bytes, the table as records of dtype `record`, the payload."""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for x, y, z, bits, payload, table in cases:
            f.write(struct.pack("<4iq", x, y, z, bits, len(payload)))
            f.write(np.ascontiguousarray(table, dtype=record).tobytes())
            f.write(payload)


def read_results(data, cases):
    """The host check's output for `cases`: per case z int32 status words, then the x*y*z words' bytes."""
    out, at = [], 0
    for x, y, z, bits, _, _ in cases:
        status = np.frombuffer(data, dtype="<i4", count=z, offset=at)
        at += 4 * z
        n = x * y * z * bits // 8
        out.append((np.frombuffer(data, dtype=np.uint8, count=n, offset=at).view(f"<u{bits // 8}").reshape(z, y, x), status))
        at += n
    assert at == len(data)
    return out


def run_host_check(tmp_path, program, cases, record):
    """tests/`program`.cpp built with the host compiler under the address and undefined-behaviour sanitizers and run, as a stand-alone
    executable, on the fixture of `cases`; its results per case, (pixels (z, y, x), status (z,))."""
    import pytest
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / program)
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", program + ".cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    fixture = str(tmp_path / "streams.bin")
    write_fixture(fixture, cases, record)
    run = subprocess.run([exe, fixture], capture_output=True, timeout=300)
    assert run.returncode == 0, run.stderr.decode("utf-8", "replace")[-4000:]
    return read_results(run.stdout, cases)


def assert_equals_restatement(name, got, want, who="device"):
    """(pixels, status) of the code under test against the restatement's, bit for bit."""
    (pixels, status), (want_pixels, want_status) = got, want
    assert np.array_equal(status, want_status), f"{name}: status {status.tolist()}, restatement {want_status.tolist()}"
    bad = np.argwhere(pixels != want_pixels)
    assert bad.shape[0] == 0, (f"{name}: {bad.shape[0]} words differ, the first at (k, j, i) = {tuple(bad[0])}: {who} "
                               f"{int(pixels[tuple(bad[0])]):#x}, restatement {int(want_pixels[tuple(bad[0])]):#x}")
    return pixels, status


# ---- refusals before any launch (no GPU: the pointers are fake and never dereferenced) ------------------------------------------------
def built_lib():
    from mmnn_sts_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.lib()


PAY, TAB, PIX, STA, WS = 0x7F0000100000, 0x7F0000200000, 0x7F0000900000, 0x7F0000080000, 0x7F0001000000     # far apart, 256-byte aligned
GOOD = dict(x=8, y=4, z=2, bits_allocated=16, payload_bytes=4096)


def bad_calls(table, too_deep):
    """{name: (descriptor fields over GOOD, (payload, table, pixels, status, workspace), reason)}.  `table`: what the call names its
    records; `too_deep`: the smallest power-of-two bit depth it does not take."""
    ok = (PAY, TAB, PIX, STA, WS)
    return {
        "null payload": ({}, (0, TAB, PIX, STA, WS), "null"), f"null {table}": ({}, (PAY, 0, PIX, STA, WS), "null"),
        "null pixels": ({}, (PAY, TAB, 0, STA, WS), "null"), "null status": ({}, (PAY, TAB, PIX, 0, WS), "null"),
        "null workspace": ({}, (PAY, TAB, PIX, STA, 0), "null"),
        "zero extent": (dict(x=0), ok, "non-positive extent"), "negative extent": (dict(z=-1), ok, "non-positive extent"),
        "2^31 voxels": (dict(x=2048, y=2048, z=512), ok, "2\\^31"),
        "bits_allocated 12": (dict(bits_allocated=12), ok, "bits_allocated"),
        f"bits_allocated {too_deep}": (dict(bits_allocated=too_deep), ok, "bits_allocated"),
        "bits_allocated 1": (dict(bits_allocated=1), ok, "bits_allocated"),
        "no payload bytes": (dict(payload_bytes=0), ok, "payload_bytes"),
        "payload misaligned": ({}, (PAY + 8, TAB, PIX, STA, WS), "payload not aligned"),
        f"{table} misaligned": ({}, (PAY, TAB + 4, PIX, STA, WS), f"{table} not aligned"),
        "pixels misaligned": ({}, (PAY, TAB, PIX + 1, STA, WS), "pixels not aligned"), "status misaligned": ({}, (PAY, TAB, PIX, STA + 2, WS), "status not aligned"),
        "workspace misaligned": ({}, (PAY, TAB, PIX, STA, WS + 8), "workspace not aligned"),
        "pixels inside payload": ({}, (PAY, TAB, PAY + 64, STA, WS), "payload and pixels overlap"),
        "payload inside pixels": ({}, (PIX + 32, TAB, PIX, STA, WS), "payload and pixels overlap"),
        "status inside payload": ({}, (PAY, TAB, PIX, PAY + 4092, WS), "payload and status overlap"),
    }


def assert_refused(lib, entry, desc_type, fields, pointers, reason):
    import pytest
    from mmnn_sts_amd import _lib
    desc = desc_type(**dict(GOOD, **fields))
    assert getattr(lib, entry)(ctypes.byref(desc), *(p or None for p in pointers), None) == 1
    with pytest.raises(ValueError, match=reason):
        _lib.check(1, entry)


# ---- the call on the device ---------------------------------------------------------------------------------------------------------------
def guarded(content, lead=GUARD):
    """A device buffer of `content` (uint8 array, or a byte count to leave patterned) between two patterned guards; (buffer, lead, size)."""
    import torch
    n = content if isinstance(content, int) else content.size
    buf = torch.full((lead + n + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
    if not isinstance(content, int):
        buf[lead:lead + n] = torch.from_numpy(np.array(content, dtype=np.uint8)).to(DEV)
    return buf, lead, n


def guarded_call(entry, desc_type, table_name, table, payload, x, y, z, bits):
    """The kernel's (pixels (z, y, x), status (z,)) for `entry`, mmnn_rle_expand or mmnn_jpegll_decode, on `payload` (bytes) and
    `table` (the records' bytes as a uint8 array).  Payload, table, pixels, status and workspace each sit inside a larger buffer: the
    inputs must come back unchanged, the guards of all five must keep their pattern."""
    import torch
    from mmnn_sts_amd import _lib
    B = bits // 8
    pay = np.frombuffer(payload, dtype=np.uint8)
    workspace = entry.rsplit("_", 1)[0] + "_workspace_bytes"
    bufs = {"payload": guarded(pay), table_name: guarded(table), "pixels": guarded(x * y * z * B), "status": guarded(4 * z),
            "workspace": guarded(_lib.count(workspace, x, y, z, bits))}
    ptr = {k: b.data_ptr() + lead for k, (b, lead, _) in bufs.items()}
    desc = desc_type(x, y, z, bits, pay.size)
    _lib.check(getattr(_lib.lib(), entry)(ctypes.byref(desc), ptr["payload"], ptr[table_name], ptr["pixels"], ptr["status"], ptr["workspace"],
                                          torch.cuda.current_stream().cuda_stream), entry)
    torch.cuda.synchronize()
    host = {k: b.cpu().numpy() for k, (b, _, _) in bufs.items()}
    for k, (_, lead, n) in bufs.items():
        assert (host[k][:lead] == PATTERN).all() and (host[k][lead + n:] == PATTERN).all(), f"bytes outside `{k}` were written"
    assert np.array_equal(host["payload"][GUARD:GUARD + pay.size], pay) and np.array_equal(host[table_name][GUARD:GUARD + table.size], table)
    inner = lambda k: host[k][bufs[k][1]:bufs[k][1] + bufs[k][2]]
    return inner("pixels").view(f"<u{B}").reshape(z, y, x), inner("status").view("<i4")


def dataset(tree):
    from mmnn_sts_amd.data.ImageDatasets import T1T2SurvivalDataset
    return T1T2SurvivalDataset(os.path.join(tree["image_loc"], "t1"), os.path.join(tree["image_loc"], "t2"), tree["data_loc"], tree["key_loc"])
