"""CPU checks of the plane-sweep backward's boundary (include/sgcdet_amd_train.h) and of its A/B partner: the header's
symbols equal the training binding table, the hipcc-built library exports them, the table stays apart from
include/sgcdet_amd.h (which the CPU oracle mirrors), and the CPU autograd of plugin ``homo_warping`` + the cost-volume
loop reproduces the reference's gradients (tests/golden/plane_sweep_grad.npz)."""
import os
import re

import torch

from plane_sweep_grad_contract import golden_cases, reference_correlation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sgc_[a-z0-9_]+)\s*\(", text)))


def test_train_header_symbols_match_train_binding_table():
    from sgcdet_amd._abi import TRAIN_SIGNATURES, TRAIN_INTROSPECTION
    assert _declared("sgcdet_amd_train.h") == sorted(list(TRAIN_SIGNATURES) + list(TRAIN_INTROSPECTION))
    assert "sgc_plane_sweep_corr_backward" in TRAIN_SIGNATURES
    assert "sgc_plane_sweep_corr_backward_workspace_bytes" in TRAIN_INTROSPECTION


def test_train_table_does_not_overlap_the_oracle_mirrored_header():
    from sgcdet_amd._abi import SIGNATURES, INTROSPECTION, TRAIN_SIGNATURES, TRAIN_INTROSPECTION
    train = set(TRAIN_SIGNATURES) | set(TRAIN_INTROSPECTION)
    assert not train & set(_declared("sgcdet_amd.h"))
    assert not train & (set(SIGNATURES) | set(INTROSPECTION))
    assert '#include "sgcdet_amd.h"' in open(os.path.join(ROOT, "include", "sgcdet_amd_train.h")).read()


def test_hip_library_exports_the_training_entry_points():
    from sgcdet_amd import build
    from sgcdet_amd._abi import Library
    lib = Library(build.build(), train=True)          # raises ImportError on a missing symbol
    assert lib.backend == "hip-gfx950"
    # the workspace query is host code: list of (source row, coefficient) entries for every corner, 8 bytes each
    N, K, H, W, D = 40, 2, 60, 80, 12
    nbytes = lib._dll.sgc_plane_sweep_corr_backward_workspace_bytes(N, K, H, W, D)
    assert 8 * N * K * H * W * D * 4 <= nbytes < 8 * N * K * H * W * D * 4 * 1.1
    assert lib._dll.sgc_plane_sweep_corr_backward_workspace_bytes(0, K, H, W, D) == 0
    # the default (oracle-compatible) binding leaves the training table alone
    assert Library(build.LIB)._dll.sgc_plane_sweep_corr_backward.argtypes is None


def test_cpu_autograd_of_the_reference_formulation_reproduces_the_golden_gradients():
    cases = golden_cases()
    assert len(cases) == 5
    for k, (f_mvs, nbr, rel, depth, grad_corr, want) in enumerate(cases):
        f = f_mvs.clone().requires_grad_(True)
        corr = reference_correlation(f, nbr, rel, depth)
        corr.backward(grad_corr)
        scale = float(want.abs().max())
        assert float((f.grad - want).abs().max()) <= 1e-5 * scale, k
    # the last case has a pixel count that is not a multiple of 64
    assert cases[4][0].shape[2] * cases[4][0].shape[3] % 64 != 0
