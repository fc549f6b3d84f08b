"""Case list of the MLP row-dropout parity (tests/test_ops_gpu.py) and the CPU rule its seeds are chosen by (tests/test_dropout_cpu.py).

Batch norm over two to four rows of which some are dropped (all-zero) rows is ill-conditioned in the way DESIGN.md 6 finding 1
describes: a tiny spread between the surviving rows is divided by its own size, and fp32 and fp64 evaluations of the SAME formula then
differ by more than any kernel error.  So the dropout seeds of the small batches are chosen (here, on the CPU, from the restated masks)
such that torch's own fp32 evaluation stays inside the comparison's tolerance of its fp64 one.  The tolerances are the ones
tests/test_fusion_gpu.py uses for the MLP without dropout: 2e-5 on outputs and running statistics (test_mlp_golden), and for the
gradients the per-tensor bound of `_compare_all_grads`, |err| <= 1e-3 |g| + 1e-5 |g_all|.  (test_mlp_golden's element-wise gradient
bound, atol = 3e-6, is an absolute number made for N = 2 / 8: the bias of a Linear in front of a batch norm has an analytically zero
gradient, and at N = 64 torch's own fp32 round-off on it is 1.3x that bound with dropout off.)  `python -m tests._dropout_cases` prints the first seeds that qualify."""
from dataclasses import dataclass

import numpy as np
import torch

from oracle import restatement as R
from oracle import synth
from tests import _util as U

TOL_OUT = 2e-5                       # rel_err of outputs and running statistics (test_mlp_golden)
GRAD_REL, GRAD_GLOBAL = 1e-3, 1e-5   # per gradient tensor: |err|_2 <= GRAD_REL * |g|_2 + GRAD_GLOBAL * |all gradients|_2
SCHEMA = R.mlp_schema(U.N_CLIN, 2, 12)
PARAM_KEYS = [k for k in SCHEMA if "running" not in k and "num_batches" not in k and not k.startswith("output_head")]
RUN_KEYS = [k for k in SCHEMA if "running" in k]


@dataclass(frozen=True)
class MlpCase:
    n: int
    p: float
    seed0: int      # stream of the `backbone` stack (layers 0..4, first_layer_id 0)
    seed1: int      # stream of the `features` stack (layer 5, first_layer_id 5)

    def masks(self):
        m = [U.mlp_row_mask_ref(self.seed0, i, self.n, self.p) for i in range(5)] + [U.mlp_row_mask_ref(self.seed1, 5, self.n, self.p)]
        return [torch.from_numpy(t).double() for t in m]


def _seeds(n, p, k):
    """Candidate k of (n, p): two full 64-bit values (the top bit set in the first, as ops.next_seed() produces them)."""
    base = (n * 0x9E3779B97F4A7C15 + int(p * 1000) * 0xD1B54A32D192ED03 + k * 0xA24BAED4963EE407) & 0xFFFFFFFFFFFFFFFF
    return base | (1 << 63), (base * 0xBF58476D1CE4E5B9 + 1) & 0x7FFFFFFFFFFFFFFF


def _params(which):
    if which == "mlp":
        return U.synth_sd(SCHEMA, "mlp.")
    # the clinical model of the fusion network of tests/test_fusion_gpu.py
    return R.sub_dict(U.synth_sd(R.multimodal_schema(R.DenseNetCfg(), U.N_CLIN, 2, 12), "fusion."), "clinical_model.model.")


def oracle(case, dtype, relu_masks=None, params="mlp"):
    """(features, dx, {param: grad}, {running}) of the training forward + backward of sum(features * cot) in `dtype`."""
    sd = {k: (v.to(dtype).requires_grad_("running" not in k) if v.is_floating_point() else v.clone()) for k, v in _params(params).items()}
    x = U.clin_in(case.n).to(dtype).requires_grad_(True)
    f = R.mlp_features(sd, x, True, case.p, drop_masks=[m.to(dtype) for m in case.masks()], relu_masks=relu_masks)
    cot = torch.from_numpy(synth.uniform("mlp/drop/cot", tuple(f.shape))).to(dtype)
    (f * cot).sum().backward()
    return f.detach(), x.grad, {k: sd[k].grad for k in PARAM_KEYS}, {k: sd[k].detach() for k in RUN_KEYS}


def worst_ratio(got, ref):
    """Largest err / tolerance over everything the GPU test compares; < 1 means every comparison passes."""
    f, dx, grads, run = got
    f64, dx64, grads64, run64 = ref
    worst = [(U.rel_err(f.double().numpy(), f64.numpy()) / TOL_OUT, "features")]
    worst += [(U.rel_err(run[k].double().numpy(), run64[k].numpy()) / TOL_OUT, k) for k in RUN_KEYS]
    pairs = [("dx", dx, dx64)] + [(k, grads[k], grads64[k]) for k in PARAM_KEYS]
    gl2 = float(np.sqrt(sum(float((r ** 2).sum()) for _, _, r in pairs)))
    for k, g, r in pairs:
        worst.append((float((g.double() - r).norm()) / (GRAD_REL * float(r.norm()) + GRAD_GLOBAL * gl2), k))
    return max(worst)


def fp32_vs_fp64(case, params="mlp"):
    return worst_ratio(oracle(case, torch.float32, params=params), oracle(case, torch.float64, params=params))[0]


def well_formed(case):
    m = case.masks()
    return any(float(t.min()) == 0.0 for t in m) and all(float(t.max()) > 0.0 for t in m)     # a dropped row; no layer loses every row


def search(n, p, margin=0.25):
    for k in range(10000):
        case = MlpCase(n, p, *_seeds(n, p, k))
        if well_formed(case) and (n > 4 or fp32_vs_fp64(case) < margin):
            return k, case
    raise AssertionError((n, p))


# candidate index per (N, p), found by search() (N <= 4: the first whose fp32 oracle is within a quarter of the tolerance of the fp64 one)
PICKED = {(2, 0.5): 17, (4, 0.5): 1}
CASES = [MlpCase(n, p, *_seeds(n, p, PICKED.get((n, p), 0))) for p in (0.2, 0.5) for n in (2, 4, 7, 64)]


def fusion_seeds(torch_seed):
    """The stream ids ops.next_seed() hands out after torch.manual_seed(torch_seed) with a fresh call counter, in the order the fusion
    model's training forward draws them: backbone (Dropout3d), image features (Dropout), MLP `backbone` stack, MLP `features` stack."""
    from mmnn_sts_amd import ops
    saved_seed, saved_counter = torch.initial_seed(), ops._seed_counter[0]
    try:
        torch.manual_seed(torch_seed)
        ops._seed_counter[0] = 0
        return [ops.next_seed() for _ in range(4)]
    finally:
        torch.manual_seed(saved_seed)
        ops._seed_counter[0] = saved_counter


def fusion_mlp_case(torch_seed, n=4, p=0.2):
    s = fusion_seeds(torch_seed)
    return MlpCase(n, p, s[2], s[3])


# torch.manual_seed of the full-step dropout test (tests/test_fusion_gpu.py, N = 4): the first value whose clinical-MLP masks are well
# formed and whose fp32 oracle is within a quarter of the tolerance of the fp64 one (same rule as above; found by the search below)
FUSION_TORCH_SEED = 0

if __name__ == "__main__":
    for ts in range(100):
        case = fusion_mlp_case(ts)
        if well_formed(case) and fp32_vs_fp64(case, "fusion") < 0.25:
            print("fusion torch seed", ts, fp32_vs_fp64(case, "fusion"))
            break
    for p in (0.2, 0.5):
        for n in (2, 4, 7, 64):
            k, case = search(n, p)
            print((n, p), k, fp32_vs_fp64(case))
