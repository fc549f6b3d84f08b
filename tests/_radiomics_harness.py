"""What the five tests/test_radiomics*_gpu.py share: uploads at a byte lead, buffers between guard bytes and the check that nothing
outside them was written, the first call and a follow-on call through the C-ABI (`radiomics.enqueue`) into such buffers, the walk over
the refusals of a follow-on call, the MLP at a table's width, the fresh-process runner and the fixture that puts the
dropout seed counter back.  The sizes of the blocks and tables stay spelt out in each test file: they are part of what it checks."""
import ctypes
import os

import numpy as np
import pytest
import torch

from mmnn_sts_amd import _lib, radiomics
from mmnn_sts_amd.data import ingest
from tests._cli import run_python

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
GUARD = 256
PATTERN = 0xA5
STAGE = {st.name: st for st in radiomics.STAGES}
GOOD_DESC = dict(x=4, y=4, z=4, scan_type=4, mask_type=2, scan_slope=1.0, scan_inter=0.0, mask_slope=1.0, mask_inter=0.0, bin_width=25.0, max_bins=16)


@pytest.fixture(autouse=True)
def leave_the_dropout_stream_where_it_was():
    """`ops.next_seed` numbers the dropout streams of the process with one counter, and the fused MLP draws from it in every forward,
    dropout or not.  Tests later in the suite restate the masks of the seeds they draw and hold fp32 gradients to tight bars, so which
    masks they get is part of what they were tuned on: the tests of a module that imports this fixture put the counter back."""
    from mmnn_sts_amd import ops
    before = ops._seed_counter[0]
    yield
    ops._seed_counter[0] = before


def device_bytes(arr, lead):
    """(holder, pointer): the array's bytes, x fastest, `lead` bytes past a 256-byte boundary."""
    host = ingest._host_bytes(np.ascontiguousarray(arr))
    buf = torch.zeros(lead + host.size + 64, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    buf[lead:lead + host.size] = torch.from_numpy(host.copy()).to(DEV)
    return buf, buf.data_ptr() + lead


def guarded(sizes):
    """(buffer, offsets): a buffer filled with PATTERN in which blocks of `sizes` bytes start on 256-byte boundaries with at least GUARD
    bytes before, between and behind them."""
    offs, off = [], GUARD
    for s in sizes:
        offs.append(off)
        off += (s + GUARD + 255) // 256 * 256
    return torch.full((off,), PATTERN, dtype=torch.uint8, device=DEV), offs


def cut(buf, offs, sizes, written):
    """The blocks of a `guarded` buffer as host bytes, once every byte outside them still holds PATTERN (`written` names them)."""
    b = buf.cpu().numpy()
    keep = np.ones(b.size, dtype=bool)
    for o, s in zip(offs, sizes):
        keep[o:o + s] = False
    assert (b[keep] == PATTERN).all(), written
    return [b[o:o + s].copy() for o, s in zip(offs, sizes)]


def _point(r, stage, buf, offs, sizes, workspace):
    attrs = STAGE[stage].attrs
    for a, o, s in zip(attrs, offs, sizes):
        setattr(r, a, buf[o:o + s])
    setattr(r, attrs[-1], workspace)


def first_call(c, guard=False):
    """`mmnn_radiomics` of a case through the C-ABI itself, enqueued on the current stream: scan and mask uploaded at their leads, the
    workspace filled with 0xFF, the result block, hist and glcm in a buffer filled with PATTERN -- between guard bytes with `guard`, behind
    each other without.  Returns (the RadiomicsResult whose tensors are views of that buffer, the descriptor, the buffer, the offsets and
    sizes of the three)."""
    x, y, z = c["scan"].shape
    mb = c["max_bins"]
    sizes = [_lib.RADIOMICS_RESULT_BYTES, mb * 4, 13 * mb * mb * 4]
    if guard:
        buf, offs = guarded(sizes)
    else:
        buf, offs = torch.full((sum(sizes),), PATTERN, dtype=torch.uint8, device=DEV), [0, sizes[0], sizes[0] + sizes[1]]
    sbuf, sp = device_bytes(c["scan"], c["scan_lead"])
    mbuf, mp = device_bytes(c["mask"], c["mask_lead"])
    ws = torch.full((radiomics.workspace_bytes(x, y, z, mb),), 0xFF, dtype=torch.uint8, device=DEV)
    desc = _lib.RadiomicsDesc(x, y, z, ingest.TYPE_CODES[c["scan"].dtype], ingest.TYPE_CODES[c["mask"].dtype], *c["scan_scale"], *c["mask_scale"],
                              c["bin_width"], mb)
    r = radiomics.RadiomicsResult(None, None, None, None, (x, y, z), None, c["bin_width"], mb)
    r.uploads = (sbuf, mbuf)                                # held until the caller has synchronised
    _point(r, "first", buf, offs, sizes, ws)
    radiomics.enqueue(r, "first", desc, torch.cuda.current_stream().cuda_stream, sp, mp)
    return r, desc, buf, offs, sizes


def follow_call(r, desc, stage, sizes, behind=0):
    """A follow-on call (`texture`, `zones`, `mesh`) behind `first_call` on the current stream: its result block and tables, of `sizes`
    bytes in the order of the C arguments, between guard bytes in one buffer filled with PATTERN; its workspace filled with 0xFF, with
    `behind` more such bytes behind it.  Returns (the buffer, the offsets, the workspace, its size without `behind`)."""
    x, y, z = r.shape
    nbytes = getattr(_lib.lib(), STAGE[stage].symbol + "_workspace_bytes")(x, y, z, r.max_bins)
    assert nbytes > 0
    ws = torch.full((nbytes + behind,), 0xFF, dtype=torch.uint8, device=DEV)
    buf, offs = guarded(sizes)
    _point(r, stage, buf, offs, sizes, ws)
    radiomics.enqueue(r, stage, desc, torch.cuda.current_stream().cuda_stream)
    return buf, offs, ws, nbytes


def refusal_walk(call, ptrs, steps, bad_descs, t):
    """The refusals every follow-on call makes before it launches anything: `call(descriptor or None, pointers)` -> status.  `bad_descs`:
    changes to GOOD_DESC that must be refused; then the null descriptor, each of `ptrs` null in turn, and each (index, bytes) of `steps`
    misaligned, with the cause in the message; at the end the zeroed buffer `t` the pointers lie in holds nothing."""
    for bad in bad_descs:
        assert call(ctypes.byref(_lib.RadiomicsDesc(**dict(GOOD_DESC, **bad))), ptrs) == 1 and _lib.last_error(), bad
    desc = ctypes.byref(_lib.RadiomicsDesc(**GOOD_DESC))
    assert call(None, ptrs) == 1 and "null" in _lib.last_error()
    for k in range(len(ptrs)):
        assert call(desc, [None if q == k else v for q, v in enumerate(ptrs)]) == 1 and "null" in _lib.last_error(), k
    for k, step in steps:
        assert call(desc, [v + step if q == k else v for q, v in enumerate(ptrs)]) == 1 and "misaligned" in _lib.last_error(), k
    torch.cuda.synchronize()
    assert not t.any()                                     # refused before any launch: nothing was written


def mlp_at_width(width, stream):
    """MLP(width) forward and backward at N = 4, training mode, against the fp64 torch restatement (oracle.restatement.mlp_features for the
    features; its layer-by-layer twin in tests/test_tail_ops_gpu.py for the gradients), at the bar that file holds width 32 to.  `stream`:
    the index of the input stream, by the rule written beside the MLP_STREAM tables of the _radiomics_*_cases.py modules."""
    from mmnn_sts_amd.models.mlp import MLP
    from oracle import restatement as OR
    from tests import test_tail_ops_gpu as TT
    from tests._util import synth_sd
    sd = synth_sd(OR.mlp_schema(width, 2, 12), f"radmlp{width}.")
    x, cot = TT._u(f"rad/mlp/x/{width}/{stream}", (4, width)), TT._u(f"rad/mlp/cot/{width}", (4, 12))
    ref, leaves, pres = TT.mlp_ref(sd, x, True)
    TT._assert_off_branch(pres, f"mlp width {width}")
    assert torch.allclose(ref.detach(), OR.mlp_features({k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}, x.double(), True, 0.0).detach(),
                          rtol=1e-12, atol=1e-14)
    (ref * cot.double()).sum().backward()
    m = MLP(width, 2, 12, dropout_prob=0.0)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).train()
    xg = x.to(DEV).requires_grad_(True)
    f = m.features(m.backbone(xg))
    (f * cot.to(DEV)).sum().backward()
    params = dict(m.named_parameters())
    errs = {"features": TT.rel_err(f.detach().cpu().numpy(), ref.detach().numpy()), "dx": TT.rel_err(xg.grad.cpu().numpy(), leaves["x"].grad.numpy())}
    for k in TT.MLP_PARAM_KEYS:
        errs[k] = TT.mlp_grad_err(k, params[k].grad, leaves, True)
    assert len(errs) == 26
    TT._check(errs, TT.BAR)


def process(argv, cwd):
    """A python command line of the package in a fresh process -> its output (`tests._cli.run_python`, five minutes at the most)."""
    return run_python(argv, cwd, limit_s=300)
