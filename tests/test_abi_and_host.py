"""CPU-side checks: the C-ABI library loads and exports exactly what include/seg2eye_hip.h declares;
host logic (options, synthetic data, state-dict compatibility, flat Adam arenas, fail-loud on CPU)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, manifest_of


def _header_symbols():
    text = open(os.path.join(ROOT, 'include', 'seg2eye_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(s2e_[a-z0-9_]+)\s*\(', text)))


def test_library_exports_every_declared_symbol():
    from seg2eye_amd import _lib
    import __graft_entry__
    __graft_entry__.build()                       # hipcc cross-compiles gfx950 without a GPU
    assert os.path.exists(_lib.LIB_PATH)
    declared = _header_symbols()
    assert len(declared) >= 20
    assert sorted(_lib.SIGNATURES) == declared, set(_lib.SIGNATURES) ^ set(declared)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    L = _lib.lib()
    assert L.s2e_version() >= 1
    assert L.s2e_conv_cout_pad(1) == 32 and L.s2e_conv_cout_pad(64) == 64 and L.s2e_conv_cout_pad(200) == 256
    assert L.s2e_conv_k_pad(_lib.S2E_BF16, 9 * 128) == 1152 and L.s2e_conv_k_pad(_lib.S2E_F32, 80) == 96


def test_every_library_switch_is_listed_in_design():
    """Every S2E_* name the library reads goes through the s2e_env_* readers of csrc/common.h (no other getenv) and stands in
    DESIGN.md's switch section, the one list of the library's switches."""
    csrc = os.path.join(ROOT, 'seg2eye_amd', 'csrc')
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    section = design[design.index('## 4. Experiment switches'):design.index('## 5. ')]
    listed = set(re.findall(r'S2E_[A-Z0-9_]+', section))
    read = set()
    for name in sorted(os.listdir(csrc)):
        text = open(os.path.join(csrc, name)).read()
        stray = [ln for ln in text.splitlines() if 'getenv(' in ln and not (name == 'common.h' and 's2e_env_' in ln)]
        assert not stray, (name, stray)
        read |= set(re.findall(r's2e_env_[a-z_]+\(\s*"(S2E_[A-Z0-9_]+)"', text))
        if name != 'common.h':                                  # outside the readers the name is always a literal
            assert len(re.findall(r's2e_env_[a-z_]+\(', text)) == len(re.findall(r's2e_env_[a-z_]+\(\s*"S2E_', text)), name
    assert len(read) >= 20, read                            # (a floor against a pattern that stopped matching)
    assert read <= listed, sorted(read - listed)


def test_argument_errors_are_reported_without_a_gpu():
    from seg2eye_amd import _lib
    L = _lib.lib()
    assert L.s2e_colsum(_lib.S2E_BF16, None, 10, 8, None, None) == -1          # S2E_ERR_ARG before any launch
    assert b's2e_colsum' in L.s2e_last_error()
    d = _lib.ConvDesc(1, 8, 8, 8, 8, 8, 8, 3, 3, 3, 1, 0, 0, 0, 0)             # stride 3 unsupported
    assert L.s2e_conv2d(_lib.S2E_BF16, 1, 1, None, None, None, 1, ctypes.byref(d), None, 0, None) == -3
    d2 = _lib.ConvDesc(8, 8, 8, 1024, 8, 8, 1024, 3, 3, 1, 1, 0, 0, 0, 0)         # small M, K = 9216: split-K
    assert L.s2e_conv2d_workspace_bytes(_lib.S2E_BF16, ctypes.byref(d2)) == 16 * 512 * 1024 * 4
    assert L.s2e_conv2d(_lib.S2E_BF16, 1, 1, None, None, None, 1, ctypes.byref(d2), None, 0, None) == -1   # workspace missing
    d3 = _lib.ConvDesc(8, 256, 256, 128, 256, 256, 256, 3, 3, 1, 1, 0, 0, 0, 0)
    assert L.s2e_conv2d_workspace_bytes(_lib.S2E_BF16, ctypes.byref(d3)) == 0
    # big bf16 3x3 layer: patch-resident weight gradient, one workgroup per CU (256 when no device is visible), each
    # storing its 9 x 128 x 64 fp32 partial tile; the fp32 build of the same shape runs the generic kernel, whose 2 x 9 dW tiles
    # x 114 pixel splits (>= 16 splits: partial tiles + a fixed-order reduction instead of atomics, round 3) each store a
    # 128 x 128 tile and 128 bias sums
    assert L.s2e_conv2d_wgrad_workspace_bytes(_lib.S2E_BF16, ctypes.byref(d3)) == 256 * 9 * 128 * 64 * 4
    assert L.s2e_conv2d_wgrad_workspace_bytes(_lib.S2E_F32, ctypes.byref(d3)) == 18 * 114 * (128 * 128 + 128) * 4
    # which kernel the library picks is a function of the shape alone (0 generic, 1 one-channel stream, 2 patch-resident)
    assert L.s2e_conv2d_kernel_kind(_lib.S2E_BF16, ctypes.byref(d3)) == 2
    assert L.s2e_conv2d_kernel_kind(_lib.S2E_F32, ctypes.byref(d3)) == 2
    assert L.s2e_conv2d_wgrad_kernel_kind(_lib.S2E_BF16, ctypes.byref(d3)) == 2
    assert L.s2e_conv2d_wgrad_kernel_kind(_lib.S2E_F32, ctypes.byref(d3)) == 0
    assert L.s2e_conv2d_kernel_kind(_lib.S2E_BF16, ctypes.byref(d2)) == 0                      # 8x8: rectangles would be 25 % full
    d4 = _lib.ConvDesc(8, 256, 256, 64, 256, 256, 1, 3, 3, 1, 1, 0, 0, 0, 0)
    assert L.s2e_conv2d_kernel_kind(_lib.S2E_BF16, ctypes.byref(d4)) == 1                      # conv_img: Cout = 1
    d5 = _lib.ConvDesc(8, 16, 16, 1024, 16, 16, 1024, 3, 3, 1, 1, 0, 0, 0, 0)                  # few tiles, long K: patch kernel, 64-channel tiles split 2x
    assert L.s2e_conv2d_kernel_kind(_lib.S2E_BF16, ctypes.byref(d5)) == 2                      # (round 5; 128-channel tiles split 4x before: twice the fp32 slabs)
    assert L.s2e_conv2d_workspace_bytes(_lib.S2E_BF16, ctypes.byref(d5)) == 2 * 8 * 16 * 16 * 1024 * 4
    d4 = _lib.ConvDesc(8, 256, 256, 64, 256, 256, 1, 3, 3, 1, 1, 0, 0, 0, 0)      # conv_img: 1-channel stream kernels
    assert L.s2e_conv2d_wgrad_workspace_bytes(_lib.S2E_BF16, ctypes.byref(d4)) == 1024 * 9 * 64 * 4
    assert L.s2e_conv2d_wgrad(_lib.S2E_BF16, 1, 1, 1, None, ctypes.byref(d4), None, 0, None) == -1        # workspace missing
    with pytest.raises(_lib.Seg2EyeHipError):
        _lib.check(-1, 'x')


def test_round6_planners_are_host_only():
    """The shape planners of round 6's kernels answer without a GPU: which launches conv_plane.hip takes (and in which mode), the
    size of a PLANE-layout weight, which weight gradients the multi-job launch takes; argument errors before any launch."""
    from seg2eye_amd import _lib
    L = _lib.lib()
    bf, f32 = _lib.S2E_BF16, _lib.S2E_F32
    mode = lambda *a: L.s2e_conv2d_plane_supported(bf, ctypes.byref(_lib.ConvDesc(*a)))
    # netE at the benchmark's size: batch 32, 3x3 stride 2 pad 1 (forward = mode 3, data gradient = mode 4)
    assert mode(32, 128, 128, 64, 64, 64, 128, 3, 3, 2, 1, 0, 0, 0, 0) == 3
    assert mode(32, 64, 64, 128, 128, 128, 64, 3, 3, 2, 1, 1, 0, 0, 0) == 4
    assert mode(32, 16, 16, 512, 8, 8, 512, 3, 3, 2, 1, 0, 0, 0, 0) == 0                # an 8 x 8 map: no 8 x 16 rectangle
    # the learned 1x1 shortcuts (mode 1), forward and data gradient
    assert mode(8, 256, 256, 128, 256, 256, 64, 1, 1, 1, 0, 0, 0, 0, 0) == 1
    assert mode(8, 256, 256, 64, 256, 256, 128, 1, 1, 1, 0, 1, 0, 0, 0) == 1
    # the PatchGAN's 4x4 stride-2 pad-2 layers on ragged maps (modes 5 / 6); its 8-channel first layer stays generic
    assert mode(16, 129, 129, 64, 65, 65, 128, 4, 4, 2, 2, 0, 0, 0, 0) == 5
    assert mode(8, 65, 65, 128, 129, 129, 64, 4, 4, 2, 2, 1, 0, 0, 0) == 6
    assert mode(16, 256, 256, 8, 129, 129, 64, 4, 4, 2, 2, 0, 0, 1, 0) == 0
    # 3x3 stride 1 stays in conv_duo.hip by default; fp32 never runs here
    assert mode(8, 128, 128, 256, 128, 128, 128, 3, 3, 1, 1, 0, 0, 0, 0) == 0
    assert L.s2e_conv2d_plane_supported(f32, ctypes.byref(_lib.ConvDesc(8, 256, 256, 128, 256, 256, 64, 1, 1, 1, 0, 0, 0, 0, 0))) == 0
    d = _lib.ConvDesc(32, 128, 128, 64, 64, 64, 200, 3, 3, 2, 1, 0, 0, 0, 0)
    assert L.s2e_conv_plane_weight_elems(ctypes.byref(d)) == 256 * 9 * 64                # rows padded to 64
    assert L.s2e_conv2d_plane(bf, 1, 1, None, None, None, 1, ctypes.byref(_lib.ConvDesc(8, 8, 8, 64, 8, 8, 64, 3, 3, 1, 1, 0, 0, 0, 0)), None) == -3
    assert b's2e_conv2d_plane' in L.s2e_last_error()
    assert L.s2e_conv2d_plane(bf, None, 1, None, None, None, 1, ctypes.byref(d), None) == -1
    # multi-job generic weight gradient: generic bf16 shapes only
    multi = lambda *a: L.s2e_conv2d_wgrad_multi_supported(bf, ctypes.byref(_lib.ConvDesc(*a)))
    assert multi(32, 128, 128, 64, 64, 64, 128, 3, 3, 2, 1, 0, 0, 0, 0) == 1             # netE stride 2
    assert multi(8, 256, 256, 128, 256, 256, 64, 1, 1, 1, 0, 0, 0, 0, 0) == 1            # 1x1 shortcut
    assert multi(8, 256, 256, 128, 256, 256, 256, 3, 3, 1, 1, 0, 0, 0, 0) == 0           # patch-resident: the batched launch's
    assert multi(8, 256, 256, 64, 256, 256, 1, 3, 3, 1, 1, 0, 0, 0, 0) == 0              # 1-channel stream kernel's
    assert L.s2e_conv2d_wgrad_multi(bf, None, 0, None, 0, None) == -1
    # ... and which of them leave the generic tile kernel for the flat-slab patch-resident one (default: the PatchGAN's 4x4 layers)
    if 'S2E_WGRAD_FLAT' not in os.environ:
        kind = lambda *a: L.s2e_conv2d_wgrad_multi_kind(bf, ctypes.byref(_lib.ConvDesc(*a)))
        assert kind(16, 129, 129, 64, 65, 65, 128, 4, 4, 2, 2, 0, 0, 0, 0) == 5          # 4x4 stride 2 on a ragged map
        assert kind(16, 33, 33, 256, 34, 34, 512, 4, 4, 1, 2, 0, 0, 0, 0) == 4           # 4x4 stride 1
        assert kind(32, 128, 128, 64, 64, 64, 128, 3, 3, 2, 1, 0, 0, 0, 0) == 0          # netE: stays generic by default
        if 'S2E_CONV_C8' not in os.environ:
            assert kind(16, 256, 256, 8, 129, 129, 64, 4, 4, 2, 2, 0, 0, 0, 0) == 6      # the PatchGAN's first layer: conv_c8.hip
            assert L.s2e_conv2d_kernel_kind(bf, ctypes.byref(_lib.ConvDesc(16, 256, 256, 8, 129, 129, 64, 4, 4, 2, 2, 0, 0, 1, 0))) == 1   # S2E_KERNEL_SMALL
        assert kind(16, 256, 256, 16, 129, 129, 64, 4, 4, 2, 2, 0, 0, 0, 0) == 0         # 16 input channels: generic
        assert kind(16, 33, 33, 256, 34, 34, 512, 4, 4, 1, 2, 0, 1, 0, 0) == 0           # an input activation: generic
        assert kind(8, 256, 256, 128, 256, 256, 256, 3, 3, 1, 1, 0, 0, 0, 0) == -1       # not a job of the multi call at all
    jobs = (_lib.WgradMultiJob * 2)()
    for j, a in zip(jobs, ((32, 128, 128, 64, 64, 64, 128, 3, 3, 2, 1, 0, 0, 0, 0), (8, 256, 256, 128, 256, 256, 64, 1, 1, 1, 0, 0, 0, 0, 0))):
        j.d = _lib.ConvDesc(*a)
    assert L.s2e_conv2d_wgrad_multi_workspace_bytes(bf, ctypes.byref(jobs), 2) % 256 == 0
    assert L.s2e_conv2d_wgrad_multi(bf, ctypes.byref(jobs), 2, None, 0, None) == -1      # null operand pointers
    assert L.s2e_shard_sum(bf, 1, 1, 8, 100, None) == -1                                  # shard bytes not a multiple of 16


def test_wgrad_multi_c8_workspace_and_argument_errors_are_host_only():
    """s2e_conv2d_wgrad_multi's c8 jobs (the PatchGAN's 8-channel first layer, conv_c8.hip) take 512 partial tiles of 64 x 128 + 64
    floats per chunk of 4 jobs, whatever the jobs' sizes; a job with a null operand is refused, naming the job, before any launch."""
    from seg2eye_amd import _lib
    if os.environ.get('S2E_CONV_C8', '1') == '0' or os.environ.get('S2E_DETERMINISTIC', '0') not in ('', '0'):
        pytest.skip('c8 kernel switched off in this environment')
    L = _lib.lib()
    bf = _lib.S2E_BF16
    tile = (64 * 128 + 64) * 4
    shapes = [(16, 128, 128), (1, 2, 2), (2, 33, 47), (1, 1, 40), (3, 17, 9), (1, 64, 64), (16, 256, 256), (1, 3, 5), (2, 20, 20)]
    for n in (4, 5, 9):
        jobs = (_lib.WgradMultiJob * n)()
        for j, (b, h, w) in zip(jobs, shapes):
            j.d = _lib.ConvDesc(b, h, w, 8, h // 2 + 1, w // 2 + 1, 64, 4, 4, 2, 2, 0, 0, 0, 0)
            assert L.s2e_conv2d_wgrad_multi_kind(bf, ctypes.byref(j.d)) == 6
        assert L.s2e_conv2d_wgrad_multi_workspace_bytes(bf, ctypes.byref(jobs), n) == -(-n // 4) * 512 * tile
        # (every pointer of every job is NULL: nothing could be launched even if the check were missing)
        assert L.s2e_conv2d_wgrad_multi(bf, ctypes.byref(jobs), n, None, 0, None) == -1
        assert b'null pointer in job 0' in L.s2e_last_error()
    # mixed table: a generic, a flat (4x4 stride 2) and a c8 job, all without operands
    jobs = (_lib.WgradMultiJob * 3)()
    for j, a in zip(jobs, ((4, 64, 64, 64, 32, 32, 128, 3, 3, 2, 1, 0, 0, 0, 0), (16, 129, 129, 64, 65, 65, 128, 4, 4, 2, 2, 0, 0, 0, 0),
                           (16, 128, 128, 8, 65, 65, 64, 4, 4, 2, 2, 0, 0, 0, 0))):
        j.d = _lib.ConvDesc(*a)
    assert L.s2e_conv2d_wgrad_multi(bf, ctypes.byref(jobs), 3, None, 0, None) == -1
    assert b'null pointer' in L.s2e_last_error()
    assert L.s2e_conv2d_wgrad_multi(bf, ctypes.byref(jobs), 4097, None, 0, None) == -1          # more than 4096 jobs


def test_pack_block_map_is_host_only():
    """s2e_pack_block_map is pure host code: grid of a forward pack = rows_pad/4 x ceil(cin_pad/64), of a
    transposed pack = ceil(cout/64) x ceil(rows_pad/8); triples are {job, bx, by}."""
    from seg2eye_amd import _lib
    L = _lib.lib()
    jobs = (_lib.PackJob * 2)()
    jobs[0].cout, jobs[0].cin, jobs[0].taps, jobs[0].cin_pad, jobs[0].transposed = 100, 70, 9, 72, 0
    jobs[1].cout, jobs[1].cin, jobs[1].taps, jobs[1].cin_pad, jobs[1].transposed = 100, 70, 9, 72, 1
    n0 = L.s2e_pack_block_map(_lib.S2E_BF16, ctypes.byref(jobs), 1, None)
    n = L.s2e_pack_block_map(_lib.S2E_BF16, ctypes.byref(jobs), 2, None)
    assert n0 == 128 // 4 * 2 and n == n0 + 2 * (128 // 8)
    bm = np.zeros(3 * n, dtype=np.int32)
    assert L.s2e_pack_block_map(_lib.S2E_BF16, ctypes.byref(jobs), 2, bm.ctypes.data) == n
    bm = bm.reshape(-1, 3)
    assert (bm[:n0, 0] == 0).all() and (bm[n0:, 0] == 1).all()
    assert bm[:n0, 1].max() == 31 and bm[:n0, 2].max() == 1 and bm[n0:, 1].max() == 1 and bm[n0:, 2].max() == 15
    assert len({tuple(r) for r in bm}) == n
    assert L.s2e_pack_conv_weights(_lib.S2E_BF16, None, None, 0, 9, None, None) == -1


def test_grad_block_map_is_host_only():
    """s2e_grad_block_map: tiles of 4 co rows x 64 ci, up to 8 tiles per block, triples {job, first tile, tiles}."""
    from seg2eye_amd import _lib
    L = _lib.lib()
    jobs = (_lib.GradJob * 2)()
    jobs[0].cout, jobs[0].cin, jobs[0].taps, jobs[0].cin_pad = 10, 130, 9, 136      # 3 row groups x 3 chunks = 9 tiles
    jobs[1].cout, jobs[1].cin, jobs[1].taps, jobs[1].cin_pad = 4, 64, 1, 64         # 1 tile
    n = L.s2e_grad_block_map(ctypes.byref(jobs), 2, None)
    assert n == 2 + 1
    bm = np.zeros(3 * n, dtype=np.int32)
    assert L.s2e_grad_block_map(ctypes.byref(jobs), 2, bm.ctypes.data) == n
    assert bm.reshape(-1, 3).tolist() == [[0, 0, 8], [0, 8, 1], [1, 0, 1]]
    assert L.s2e_weight_grads_batched(None, None, 0, 9, 0, None, None) == -1


def test_per_layer_weight_grad_entries_refuse_more_than_64_taps():
    """Like s2e_weight_grads_batched, the per-layer entries take at most 64 taps (the tile's LDS row) and say so before any launch:
    -3 is S2E_ERR_UNSUPPORTED.  (P: a dummy non-null pointer, never dereferenced.)"""
    from seg2eye_amd import _lib
    L = _lib.lib()
    P = 0x7000
    assert L.s2e_weight_grads_batched(P, P, 1, 65, 0, None, None) == -3
    assert L.s2e_last_error() == b's2e_weight_grads_batched: more than 64 taps'
    for kh, kw in ((5, 13), (65, 1), (9, 9)):
        assert L.s2e_unpack_weight_grad(P, P, 4, 64, kh, kw, 64, 0, None) == -3
        assert L.s2e_last_error() == b's2e_unpack_weight_grad: more than 64 taps'
        assert L.s2e_sn_weight_grad(P, P, P, P, P, P, P, 4, 64, kh, kw, 64, 1, None) == -3
        assert L.s2e_last_error() == b's2e_sn_weight_grad: more than 64 taps'
    assert L.s2e_unpack_weight_grad(None, P, 4, 64, 9, 9, 64, 0, None) == -1              # a bad argument wins over the size
    assert L.s2e_sn_weight_grad(P, P, P, P, P, None, P, 4, 64, 9, 9, 64, 0, None) == -1


def test_ops_refuse_cpu_tensors():
    from seg2eye_amd import ops, _lib, networks
    from seg2eye_amd.options import default_opt
    with pytest.raises(_lib.Seg2EyeHipError):
        ops.in_stats(torch.zeros(1, 4, 4, 8))
    G = networks.SPADESTYLEGenerator(default_opt(ngf=8, crop_size=64, gpu_ids=[]))
    with pytest.raises(_lib.Seg2EyeHipError):
        G(torch.zeros(1, 4, 64, 64), torch.zeros(1, 16))


def test_grad_sink_drops_every_queue_of_a_failed_step():
    """A trainer step that raises leaves nothing queued: a job surviving into the next scope would run there, on tensors of a
    step that no longer exists (the in-place chain-rule queue used to).  Host bookkeeping only: CPU tensors, no library call."""
    from seg2eye_amd import ops
    queues = ('jobs', 'inplace', 'wg', 'gwg', 'c8', 'uni')
    pool = ops.ZeroPool('cpu')
    grad, weight = torch.zeros(16, 8, 3, 3), torch.zeros(16, 8, 3, 3)
    with pytest.raises(ZeroDivisionError):
        with pool.scope('G'):
            assert ops.GradSink.push(torch.zeros(16, 72), grad, 16, 8, 9, 8)
            ops.GradSink.push_inplace(grad.view(16, 72), weight, torch.zeros(16), torch.zeros(72), torch.ones(1), 16, 8, 9)
            assert len(pool.sink.jobs) == 1 and len(pool.sink.inplace) == 1
            pool.sink.inplace_done.add(1)
            pool.sink.wg_done.add(2)
            1 // 0
    assert ops.ZeroPool.active() is None
    assert {q: len(getattr(pool.sink, q)) for q in queues} == {q: 0 for q in queues}
    with pool.scope('G'):                                    # a scope that ends normally with nothing queued
        assert pool.sink.inplace_done == set() and pool.sink.wg_done == set()
    assert ops.ZeroPool.active() is None
    assert {q: len(getattr(pool.sink, q)) for q in queues} == {q: 0 for q in queues}
    with pool.scope('D'):
        assert pool.sink.inplace_done == set() and pool.sink.wg_done == set()


def test_state_dict_layout_matches_reference():
    from seg2eye_amd import networks
    from seg2eye_amd.options import default_opt
    z = load_golden('trainer_ngf8_256')
    opt = default_opt(ngf=8, ndf=8, crop_size=256, gpu_ids=[])
    for tag, cls in (('G', networks.SPADESTYLEGenerator), ('D', networks.MultiscaleDiscriminator), ('E', networks.ConvEncoder)):
        sd = cls(opt).state_dict()
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == manifest_of(z, tag)
    big = default_opt(ngf=64, ndf=64, crop_size=256, gpu_ids=[])
    n = lambda net: sum(p.numel() for p in net.parameters())
    assert abs(n(networks.SPADESTYLEGenerator(big)) / 1e6 - 92.46) < 0.01
    assert abs(n(networks.MultiscaleDiscriminator(big)) / 1e6 - 5.53) < 0.01
    assert abs(n(networks.ConvEncoder(big)) / 1e6 - 6.53) < 0.01


def test_options_and_shapes():
    from seg2eye_amd.options import default_opt, latent_size, image_hw
    assert latent_size(default_opt(crop_size=256, aspect_ratio=1.0)) == (8, 8)
    assert image_hw(default_opt(crop_size=256, aspect_ratio=0.8)) == (320, 256)
    assert image_hw(default_opt(crop_size=384, aspect_ratio=0.6)) == (640, 384)
    with pytest.raises(ValueError):
        latent_size(default_opt(num_upsampling_layers='most'))
    with pytest.raises(KeyError):
        default_opt(not_an_option=1)
    from seg2eye_amd.pix2pix_model import Pix2PixModel
    bn = Pix2PixModel(default_opt(ngf=8, ndf=8, gpu_ids=[], norm_G='spectralspadebatch3x3'))     # the reference's default norm
    assert len(bn.netG.state_dict()) == 270 and 'head_0.norm_0.spade.param_free_norm.running_mean' in bn.netG.state_dict()
    with pytest.raises(ValueError):
        Pix2PixModel(default_opt(ngf=8, ndf=8, gpu_ids=[], norm_G='spectralspadesyncbatch3x3'))
    Pix2PixModel(default_opt(ngf=8, ndf=8, gpu_ids=[], lambda_openeds=1.0))          # built since SURVEY 8 f3 (s2e_openeds_error)
    with pytest.raises(NotImplementedError):
        Pix2PixModel(default_opt(ngf=8, ndf=8, gpu_ids=[], no_vgg_loss=False))


def test_synthetic_is_deterministic_and_wellformed():
    from seg2eye_amd import synthetic as syn
    a, b = syn.make_batch(2, 64, 64, seed=5), syn.make_batch(2, 64, 64, seed=5)
    assert all(np.array_equal(a[k], b[k]) for k in ('label', 'style_image', 'target'))
    assert a['label'].dtype == np.uint8 and a['label'].shape == (2, 1, 64, 64) and set(np.unique(a['label'])) <= {0, 1, 2, 3}
    assert len(np.unique(a['label'])) == 4
    assert a['style_image'].shape == (2, 4, 1, 64, 64) and np.abs(a['style_image']).max() <= 1.0
    assert not np.array_equal(a['label'], syn.make_batch(2, 64, 64, seed=6)['label'])
    sd = syn.fill_state_dict([('c.weight_orig', (8, 4, 3, 3)), ('c.weight_u', (8,)), ('c.weight_v', (36,)), ('c.bias', (8,))])
    wm = sd['c.weight_orig'].reshape(8, -1).astype(np.float64)
    sigma = sd['c.weight_u'] @ wm @ sd['c.weight_v']
    assert abs(sigma - np.linalg.svd(wm, compute_uv=False)[0]) < 1e-3 * sigma       # settled to the top singular pair


def test_flat_adam_arena_aliases_parameters():
    from seg2eye_amd.optim import FlatAdam
    lin = torch.nn.Linear(5, 3)
    w0 = lin.weight.detach().clone()
    opt = FlatAdam(list(lin.parameters()), lr=1e-3, betas=(0, 0.9))
    assert opt.betas == (0.0, 0.9) and isinstance(opt.betas[0], float)
    assert torch.equal(lin.weight.detach(), w0)
    assert lin.weight.data_ptr() == opt.flat_p.data_ptr() and lin.weight.grad.data_ptr() == opt.flat_g.data_ptr()
    assert all(o % 4 == 0 for o in opt.offsets) and opt.numel == 16 + 4
    lin(torch.ones(2, 5)).sum().backward()
    assert float(opt.flat_g.abs().sum()) > 0 and lin.weight.grad.data_ptr() == opt.flat_g.data_ptr()
    opt.zero_grad()
    assert float(opt.flat_g.abs().sum()) == 0
    with pytest.raises(Exception):
        opt.step()                                                                        # GPU-only kernel
    assert float(FlatAdam(list(torch.nn.Linear(2, 2).parameters()), lr=1e-3, weight_decay=0.1).hyper[6]) == pytest.approx(0.1)


def test_flat_adam_channels_last_arena_layout():
    """Conv weights with Cin % 8 == 0 are stored [Cout][KH][KW][Cin] in the arenas, 256-byte aligned, and exposed as
    (Cout,Cin,KH,KW) views: same values, state_dict unchanged; the moments' layout is tagged and a mismatching load refused."""
    from seg2eye_amd.optim import FlatAdam
    from seg2eye_amd import optim as optim_mod
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Conv2d(8, 16, 3), torch.nn.Conv2d(16, 24, 3), torch.nn.Conv2d(4, 8, 3), torch.nn.Linear(5, 3))
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    opt = FlatAdam(list(net.parameters()), lr=1e-3, channels_last=True)
    w0, w2 = net[0].weight, net[2].weight
    assert opt.cl == [True, False, True, False, False, False, False, False]            # (Cin = 4 keeps torch's order)
    assert w0.shape == (16, 8, 3, 3) and w0.stride() == (72, 1, 24, 8) and not w0.is_contiguous()
    assert w0.permute(0, 2, 3, 1).is_contiguous() and w0.grad.stride() == w0.stride() and w2.is_contiguous()
    assert all(opt.offsets[i] % 64 == 0 for i, c in enumerate(opt.cl) if c)
    assert (w0.data_ptr() - opt.flat_p.data_ptr()) % 256 == 0
    for k, v in net.state_dict().items():
        assert torch.equal(v, before[k]), k                                              # values by logical index: unchanged
    # the arena really is [co][ky][kx][ci]
    off = opt.offsets[0]
    assert torch.equal(opt.flat_p[off:off + w0.numel()].view(16, 3, 3, 8), before['0.weight'].permute(0, 2, 3, 1))
    x = torch.randn(2, 8, 12, 12)
    net[:2](x).sum().backward()                                                         # torch's own kernels accumulate into the views
    ref = torch.nn.Sequential(torch.nn.Conv2d(8, 16, 3), torch.nn.Conv2d(16, 24, 3))
    ref.load_state_dict({k: v for k, v in before.items() if k[0] in '01'})
    ref(x).sum().backward()
    assert torch.allclose(w0.grad, ref[0].weight.grad, atol=1e-5) and w0.grad.data_ptr() == opt.flat_g.data_ptr() + 4 * off
    sd = opt.state_dict()
    assert sd['layout']['channels_last'] == opt.cl
    opt.load_state_dict(sd)
    #  a state carries its parameter signature: the same parameters in another MEMORY order are converted by logical
    # index, a permuted parameter list is refused, a state without any signature is refused unless the caller vouches for its order
    opt.flat_m.copy_(torch.arange(opt.numel, dtype=torch.float32))
    opt.flat_v.copy_(torch.arange(opt.numel, dtype=torch.float32) * 0.5)
    opt.step_count = 7
    sd = opt.state_dict()
    mk = lambda: torch.nn.Sequential(torch.nn.Conv2d(8, 16, 3), torch.nn.Conv2d(16, 24, 3), torch.nn.Conv2d(4, 8, 3), torch.nn.Linear(5, 3))
    other = FlatAdam(list(mk().parameters()), lr=1e-3, channels_last=False)
    other.load_state_dict(sd)
    assert other.step_count == 7
    def same_moments(a, b):
        for i, (pa, pb) in enumerate(zip(a.params, b.params)):
            for fa, fb in ((a.flat_m, b.flat_m), (a.flat_v, b.flat_v)):
                if not torch.equal(optim_mod._arena_view(fa, a.offsets[i], pa, a.cl[i]), optim_mod._arena_view(fb, b.offsets[i], pb, b.cl[i])):
                    return False                                                          # (same moment for the same logical weight element)
        return True
    assert same_moments(opt, other)
    back = FlatAdam(list(mk().parameters()), lr=1e-3, channels_last=True)
    back.load_state_dict(other.state_dict())                                              # torch order -> channels-last
    assert same_moments(opt, back)
    prm = list(mk().parameters())
    permuted = FlatAdam([prm[2], prm[3], prm[0], prm[1]] + prm[4:], lr=1e-3, channels_last=False)
    with pytest.raises(ValueError, match='another parameter list'):
        permuted.load_state_dict(other.state_dict())
    legacy = {k: v for k, v in other.state_dict().items() if k != 'layout'}               # what S2E_WEIGHTS_CL=0 builds before round 5 wrote
    with pytest.raises(ValueError, match='no layout'):
        back.load_state_dict(legacy)
    back.flat_m.zero_()
    back.load_state_dict(legacy, trust_param_order=True)
    assert same_moments(opt, back)
    unsigned = dict(sd, layout={k: v for k, v in sd['layout'].items() if k != 'shapes'})  # round 3/4 states: layout without signature
    opt.load_state_dict(unsigned)
    with pytest.raises(ValueError, match='no parameter signature'):
        other.load_state_dict(unsigned)


def test_channels_last_pack_and_inplace_gradient_maps_are_host_only():
    """s2e_pack_block_map with the channels-last source bit (transposed | 2) and s2e_sngrad_block_map / _scratch_floats: pure
    host code."""
    from seg2eye_amd import _lib
    L = _lib.lib()
    jobs = (_lib.PackJob * 2)()
    jobs[0].cout, jobs[0].cin, jobs[0].taps, jobs[0].cin_pad, jobs[0].transposed = 256, 128, 9, 128, 2      # forward: 2048 elements per block
    jobs[1].cout, jobs[1].cin, jobs[1].taps, jobs[1].cin_pad, jobs[1].transposed = 256, 128, 9, 128, 3      # transposed: 64 x 64 tile per tap
    n0 = L.s2e_pack_block_map(_lib.S2E_BF16, ctypes.byref(jobs), 1, None)
    n = L.s2e_pack_block_map(_lib.S2E_BF16, ctypes.byref(jobs), 2, None)
    assert n0 == 256 * 1152 // 2048 and n - n0 == (256 // 64) * 9 * (128 // 64)
    sj = (_lib.SnGradJob * 2)()
    sj[0].rows, sj[0].cin, sj[0].taps = 64, 64, 9          # 36864 elements: 3 chunks of 16384
    sj[1].rows, sj[1].cin, sj[1].taps = 8, 8, 1            # 64 elements: 1 chunk
    nb = L.s2e_sngrad_block_map(ctypes.byref(sj), 2, None)
    assert nb == 4 and (sj[0].part0, sj[0].nparts, sj[1].part0, sj[1].nparts) == (0, 3, 3, 1)
    bm = np.zeros(2 * nb, dtype=np.int32)
    assert L.s2e_sngrad_block_map(ctypes.byref(sj), 2, bm.ctypes.data) == nb
    assert bm.reshape(-1, 2).tolist() == [[0, 0], [0, 1], [0, 2], [1, 0]]
    assert (sj[0].vmem0, sj[1].vmem0) == (4, 4 + 576) and L.s2e_sngrad_scratch_floats(ctypes.byref(sj), 2) == 4 + 576 + 8
    assert L.s2e_sn_grads_inplace(None, None, 0, None, None) == -1


def test_checkpoint_roundtrip_and_module_prefix(tmp_path):
    from seg2eye_amd import checkpoint, networks
    from seg2eye_amd.options import default_opt
    opt = default_opt(ngf=8, ndf=8, crop_size=64, gpu_ids=[], checkpoints_dir=str(tmp_path), name='t')
    D = networks.MultiscaleDiscriminator(opt)
    path = checkpoint.save_network(D, 'D', 'latest', opt)
    assert path.endswith('latest_net_D.pth')                                              # util/util.py:195-200
    sd = torch.load(path)
    torch.save({'module.' + k: v for k, v in sd.items()}, path)                           # DataParallel-style keys
    D2 = networks.MultiscaleDiscriminator(opt)
    checkpoint.load_network(D2, 'D', 'latest', opt)
    for (k, a), (_, b) in zip(D.state_dict().items(), D2.state_dict().items()):
        assert torch.equal(a, b), k


# A dummy (never dereferenced) non-null pointer, 16-byte aligned; the dtype codes; the S2E_NORM_* modes used below; one conv shape
# (an s2e_conv_desc, passed by reference): the patch-resident forward, the generic weight gradient.
P, BF16, F32, BAD = 0x7000, 1, 0, 7
SP, ACC = 0, 0x100
BIG = ('s2e_conv_desc', 8, 256, 256, 128, 256, 256, 256, 3, 3, 1, 1, 0, 0, 0, 0)
# (entry point, arguments, return code, s2e_last_error()) of calls that fail BEFORE any launch: per entry point a missing required
# pointer, dtype 7 with otherwise plausible arguments (and with a second fault, to pin which check wins), and where the op has a
# vector-width rule a C that breaks it for that dtype.  -1 is S2E_ERR_ARG, -3 S2E_ERR_UNSUPPORTED.
HOST_ERROR_TABLE = [
    ('s2e_label_conv3x3', (BF16, None, P, P, P, 1, 8, 8, 8, 8, 4, 16, 0, None), -1, 's2e_label_conv3x3: bad argument'),
    ('s2e_label_conv3x3', (BAD, P, P, P, P, 1, 8, 8, 8, 8, 4, 16, 0, None), -1, 's2e_label_conv3x3: bad dtype 7'),
    ('s2e_label_conv3x3', (BAD, P, P, P, P, 1, 9, 8, 8, 8, 4, 16, 0, None), -3, 's2e_label_conv3x3: 9x8 is not an integer multiple of 8x8'),
    ('s2e_label_conv3x3_batch', (BF16, P, None, P, 4, P, 1, 8, 8, 4, None), -1, 's2e_label_conv3x3_batch: bad argument'),
    ('s2e_label_conv3x3_batch', (BAD, P, P, P, 4, P, 1, 8, 8, 4, None), -1, 's2e_label_conv3x3_batch: bad dtype 7'),
    ('s2e_onehot_nhwc', (BF16, P, None, None, 1, 8, 8, 8, 8, 4, 8, None), -1, 's2e_onehot_nhwc: bad argument'),
    ('s2e_onehot_nhwc', (BAD, P, None, P, 1, 8, 8, 8, 8, 4, 8, None), -1, 's2e_onehot_nhwc: bad dtype 7'),
    ('s2e_onehot_nhwc', (BAD, P, None, P, 1, 8, 8, 8, 8, 4, 5, None), -1, 's2e_onehot_nhwc: bad dtype 7'),
    ('s2e_upsample2x_fwd', (BF16, None, P, 1, 4, 4, 8, None), -1, 's2e_upsample2x_fwd: bad argument'),
    ('s2e_upsample2x_fwd', (BAD, P, P, 1, 4, 4, 8, None), -1, 's2e_upsample2x_fwd: bad dtype 7'),
    ('s2e_upsample2x_fwd', (BF16, P, P, 1, 4, 4, 12, None), -3, 's2e_upsample2x_fwd: C=12 not a multiple of 8'),
    ('s2e_upsample2x_fwd', (F32, P, P, 1, 4, 4, 6, None), -3, 's2e_upsample2x_fwd: C=6 not a multiple of 4'),
    ('s2e_upsample2x_bwd', (F32, P, None, 1, 4, 4, 8, None), -1, 's2e_upsample2x_bwd: bad argument'),
    ('s2e_upsample2x_bwd', (BAD, P, P, 1, 4, 4, 8, None), -1, 's2e_upsample2x_bwd: bad dtype 7'),
    ('s2e_upsample2x_bwd', (BF16, P, P, 1, 4, 4, 12, None), -3, 's2e_upsample2x_bwd: C=12 not a multiple of 8'),
    ('s2e_upsample2x_bwd', (F32, P, P, 1, 4, 4, 6, None), -3, 's2e_upsample2x_bwd: C=6 not a multiple of 4'),
    ('s2e_avgpool3x3s2_fwd', (BF16, None, P, 1, 8, 8, 8, None), -1, 's2e_avgpool3x3s2_fwd: bad argument'),
    ('s2e_avgpool3x3s2_fwd', (BAD, P, P, 1, 8, 8, 8, None), -1, 's2e_avgpool3x3s2_fwd: bad dtype 7'),
    ('s2e_avgpool3x3s2_bwd', (F32, P, None, 1, 8, 8, 8, None), -1, 's2e_avgpool3x3s2_bwd: bad argument'),
    ('s2e_avgpool3x3s2_bwd', (BAD, P, P, 1, 8, 8, 3, None), -1, 's2e_avgpool3x3s2_bwd: bad dtype 7'),
    ('s2e_tanh_bwd', (BF16, P, None, P, 64, None), -1, 's2e_tanh_bwd: bad argument'),
    ('s2e_tanh_bwd', (BAD, P, P, P, 64, None), -1, 's2e_tanh_bwd: bad dtype 7'),
    ('s2e_lrelu_bwd', (BF16, P, P, None, 64, None), -1, 's2e_lrelu_bwd: bad argument'),
    ('s2e_lrelu_bwd', (BAD, P, P, P, 64, None), -1, 's2e_lrelu_bwd: bad dtype 7'),
    ('s2e_lrelu_bwd', (BAD, P, P + 4, P, 64, None), -1, 's2e_lrelu_bwd: pointers must be 16-byte aligned'),
    ('s2e_bilinear_resize_fwd', (BF16, None, P, 1, 8, 8, 4, 4, None), -1, 's2e_bilinear_resize_fwd: bad argument'),
    ('s2e_bilinear_resize_fwd', (BAD, P, P, 1, 8, 8, 4, 4, None), -1, 's2e_bilinear_resize_fwd: bad dtype 7'),
    ('s2e_bilinear_resize_fwd', (BAD, P, P, 1, 8, 8, 70000, 4, None), -1, 's2e_bilinear_resize_fwd: bad dtype 7'),
    ('s2e_bilinear_resize_bwd', (F32, P, None, 1, 8, 8, 4, 4, None), -1, 's2e_bilinear_resize_bwd: bad argument'),
    ('s2e_bilinear_resize_bwd', (BAD, P, P, 1, 8, 8, 4, 4, None), -1, 's2e_bilinear_resize_bwd: bad dtype 7'),
    ('s2e_spade_class_table', (BF16, P, P, None, P, P, 4, 64, 64, None), -1, 's2e_spade_class_table: bad argument (nh <= 128)'),
    ('s2e_spade_class_table', (BAD, P, P, P, P, P, 4, 64, 64, None), -1, 's2e_spade_class_table: bad dtype 7'),
    ('s2e_spade_class_table_batch', (F32, P, None, 4, P, 4, None), -1, 's2e_spade_class_table_batch: bad argument'),
    ('s2e_spade_class_table_batch', (BAD, P, P, 4, P, 4, None), -1, 's2e_spade_class_table_batch: bad dtype 7'),
    ('s2e_spade_modulate_uniform', (BF16, P, P, P, 0, P, P, P, None, P, None, 1, 16, 16, 64, 8, 8, 1, 0, None), -1, 's2e_spade_modulate_uniform: bad argument'),
    ('s2e_spade_modulate_uniform', (BAD, P, P, P, 0, P, P, P, P, P, None, 1, 16, 16, 64, 8, 8, 1, 0, None), -1, 's2e_spade_modulate_uniform: bad dtype 7'),
    ('s2e_spade_modulate_uniform', (BAD, P, P, P, 0, P, P, P, P, P, None, 1, 15, 16, 64, 8, 8, 1, 1, None), -1, 's2e_spade_modulate_uniform: x_up needs even H, W'),
    ('s2e_spade_modulate_uniform', (BF16, P, P, P, 0, P, P, P, P, P, None, 1, 16, 16, 12, 8, 8, 1, 0, None), -3, 's2e_spade_modulate_uniform: C=12 not a multiple of 8'),
    ('s2e_spade_modulate_uniform', (F32, P, P, P, 0, P, P, P, P, P, None, 1, 16, 16, 6, 8, 8, 1, 0, None), -3, 's2e_spade_modulate_uniform: C=6 not a multiple of 4'),
    ('s2e_spade_uniform_sums', (BF16, None, 1, 64, 64, 128, 4, P, P, P, P, None), -1, 's2e_spade_uniform_sums: null pointer'),
    ('s2e_spade_uniform_sums', (BAD, P, 1, 64, 64, 128, 4, P, P, P, P, None), -1, 's2e_spade_uniform_sums: bad dtype 7'),
    ('s2e_in_stats', (BF16, None, 1, 64, 8, 1e-05, P, P, None), -1, 's2e_in_stats: bad argument'),
    ('s2e_in_stats', (BAD, P, 1, 64, 8, 1e-05, P, P, None), -1, 's2e_in_stats: bad dtype 7'),
    ('s2e_in_stats', (BF16, P, 1, 64, 12, 1e-05, P, P, None), -3, 's2e_in_stats: C=12 not a multiple of 8'),
    ('s2e_in_stats', (F32, P, 1, 64, 6, 1e-05, P, P, None), -3, 's2e_in_stats: C=6 not a multiple of 4'),
    ('s2e_colsum', (BF16, None, 10, 8, P, None), -1, 's2e_colsum: bad argument'),
    ('s2e_colsum', (BAD, P, 10, 8, P, None), -1, 's2e_colsum: bad dtype 7'),
    ('s2e_colsum', (BAD, P, 10, 3, P, None), -1, 's2e_colsum: bad dtype 7'),
    ('s2e_modulate_fwd', (BF16, 1, P, None, None, None, P, 1, 64, 8, 0, 0, None), -1, 's2e_modulate_fwd: bad argument'),
    ('s2e_modulate_fwd', (BF16, 0, P, None, P, P, P, 1, 64, 8, 0, 0, None), -1, 's2e_modulate_fwd: SPADE_STYLE needs gb and style'),
    ('s2e_modulate_fwd', (BAD, 1, P, None, P, None, P, 1, 64, 8, 0, 0, None), -1, 's2e_modulate_fwd: bad dtype 7'),
    ('s2e_modulate_fwd', (BAD, 0, P, None, P, None, P, 1, 64, 8, 0, 0, None), -1, 's2e_modulate_fwd: SPADE_STYLE needs gb and style'),
    ('s2e_modulate_fwd', (BF16, 1, P, None, P, None, P, 1, 64, 12, 0, 0, None), -3, 's2e_modulate_fwd: C=12 not a multiple of 8'),
    ('s2e_modulate_fwd', (F32, 1, P, None, P, None, P, 1, 64, 6, 0, 0, None), -3, 's2e_modulate_fwd: C=6 not a multiple of 4'),
    ('s2e_modulate_bwd', (BF16, 1, P, P, None, None, P, None, P, None, None, None, None, 1, 64, 8, 0, 0, 0, 0.0, 0, 0, None), -1, 's2e_modulate_bwd: bad argument'),
    ('s2e_modulate_bwd', (BF16, 0, P, P, P, None, P, P, P, None, None, P, P, 1, 64, 8, 0, 0, 0, 0.0, 0, 0, None), -1, 's2e_modulate_bwd: SPADE_STYLE needs gb, style, dgb, dstyle'),
    ('s2e_modulate_bwd', (BAD, 1, P, P, None, None, P, None, P, None, None, None, P, 1, 64, 8, 0, 0, 0, 0.0, 0, 0, None), -1, 's2e_modulate_bwd: bad dtype 7'),
    ('s2e_modulate_bwd', (BF16, 1, P, P, None, None, P, None, P, None, None, None, P, 1, 64, 12, 0, 0, 0, 0.0, 0, 0, None), -3, 's2e_modulate_bwd: C=12 not a multiple of 8'),
    ('s2e_modulate_bwd', (F32, 1, P, P, None, None, P, None, P, None, None, None, P, 1, 64, 6, 0, 0, 0, 0.0, 0, 0, None), -3, 's2e_modulate_bwd: C=6 not a multiple of 4'),
    ('s2e_modulate_bwd', (BF16, 1, P, P, P, P, P, P, P, None, P, P, P, 1, 64, 8, 0, 0, 0, 0.0, 0, 0, None), -1, 's2e_modulate_bwd: out (the gamma-only form) goes with the SPADE_STYLE modes only'),
    ('s2e_modulate_bwd', (BF16, 0, P, P, None, P, P, P, P, None, P, P, P, 1, 64, 8, 0, 0, 0, 0.0, 0, 0, None), -1, 's2e_modulate_bwd: SPADE_STYLE needs gb, style, dgb, dstyle'),
    ('s2e_modulate_bwd', (BF16, 0, P, P, P, P, P, P, None, None, P, P, P, 1, 64, 8, 0, 0, 0, 0.0, 0, 0, None), -1, 's2e_modulate_bwd: bad argument'),
    ('s2e_modulate_bwd', (BAD, 0, P, P, P, P, P, P, P, None, P, P, P, 1, 64, 8, 0, 0, 0, 0.0, 0, 0, None), -1, 's2e_modulate_bwd: bad dtype 7'),
    ('s2e_modulate_bwd', (BF16, 0, P, P, P, P, P, P, P, None, P, P, P, 1, 64, 12, 0, 0, 0, 0.0, 0, 0, None), -3, 's2e_modulate_bwd: C=12 not a multiple of 8'),
    ('s2e_modulate_bwd', (F32, 0, P, P, P, P, P, P, P, None, P, P, P, 1, 64, 6, 0, 0, 0, 0.0, 0, 0, None), -3, 's2e_modulate_bwd: C=6 not a multiple of 4'),
    ('s2e_modulate_bwd', (BF16, 0, P, P, P, P, P, P, P, None, P, P, P, 1, 64, 8, 0, 0, 3, 0.0, 0, 0, None), -1, 's2e_modulate_bwd: stage 3'),
    ('s2e_modulate_bwd', (BF16, 0, P, P, P, P, None, P, P, None, P, P, P, 1, 64, 8, 0, 0, 1, 0.0, 0, 0, None), -1, 's2e_modulate_bwd: bad argument'),
    ('s2e_modulate_bwd', (BAD, 0, P, P, P, P, P, P, P, None, P, P, P, 1, 64, 8, 0, 0, 1, 0.0, 0, 0, None), -1, 's2e_modulate_bwd: bad dtype 7'),
    ('s2e_modulate_bwd', (BAD, 0, P, P, P, P, P, P, P, None, P, P, P, 1, 64, 8, 0, 0, 1, 0.0, 8, 0, None), -1, 's2e_modulate_bwd: bad dtype 7'),
    ('s2e_modulate_bwd', (BF16, 0, P, P, P, P, P, P, P, None, P, P, P, 1, 64, 12, 0, 0, 1, 0.0, 0, 0, None), -3, 's2e_modulate_bwd: C=12 not a multiple of 8'),
    ('s2e_modulate_bwd', (F32, 0, P, P, P, P, P, P, P, None, P, P, P, 1, 64, 6, 0, 0, 1, 0.0, 0, 0, None), -3, 's2e_modulate_bwd: C=6 not a multiple of 4'),
    ('s2e_modulate_bwd', (BF16, 0, P, P, P, P, P, P, P, None, P, P, P, 1, 64, 8, 0, 0, 1, 0.0, 8, 0, None), -1, 's2e_modulate_bwd: x at half resolution needs the gamma-only form, per-sample statistics and an even H x W map'),
    ('s2e_modulate_bwd', (BF16, SP | ACC, P, P, P, P, P, P, P, P + 16, P, P, P, 1, 64, 8, 0, 0, 3, 0.0, 0, 0, None), -1, 's2e_modulate_bwd: stage 3'),
    ('s2e_modulate_bwd', (BF16, 0, P, P, P, P, P, P, P, P + 16, P, P, P, 1, 64, 8, 0, 0, 0, 0.0, 0, 0, None), -1, 's2e_modulate_bwd: dx_add apart from dx needs S2E_NORM_ACCUMULATE_DX'),
    ('s2e_modulate_bwd', (BF16, SP | ACC, P, P, P, P, P, P, None, P + 16, P, P, P, 1, 64, 8, 0, 0, 0, 0.0, 0, 0, None), -1, 's2e_modulate_bwd: bad argument'),
    ('s2e_modulate_bwd', (BAD, SP | ACC, P, P, P, P, P, P, P, P + 16, P, P, P, 1, 64, 8, 0, 0, 0, 0.0, 0, 0, None), -1, 's2e_modulate_bwd: bad dtype 7'),
    ('s2e_modulate_bwd', (BF16, SP | ACC, P, P, P, P, P, P, P, P + 16, P, P, P, 1, 64, 12, 0, 0, 0, 0.0, 0, 0, None), -3, 's2e_modulate_bwd: C=12 not a multiple of 8'),
    ('s2e_modulate_bwd', (F32, SP | ACC, P, P, P, P, P, P, P, P + 16, P, P, P, 1, 64, 6, 0, 0, 0, 0.0, 0, 0, None), -3, 's2e_modulate_bwd: C=6 not a multiple of 4'),
    ('s2e_instance_norm_fwd', (BF16, P, P, P, None, 1, 64, 8, 1e-05, 1, None), -1, 's2e_instance_norm_fwd: bad argument'),
    ('s2e_instance_norm_fwd', (BAD, P, P, P, P, 1, 64, 8, 1e-05, 1, None), -1, 's2e_instance_norm_fwd: bad dtype 7'),
    ('s2e_instance_norm_fwd', (BF16, P, P, P, P, 1, 64, 12, 1e-05, 1, None), -3, 's2e_instance_norm_fwd: C=12 not a multiple of 8'),
    ('s2e_instance_norm_fwd', (F32, P, P, P, P, 1, 64, 6, 1e-05, 1, None), -3, 's2e_instance_norm_fwd: C=6 not a multiple of 4'),
    ('s2e_instance_norm_bwd', (BF16, P, P, None, P, P, 1, 64, 8, 1, None), -1, 's2e_instance_norm_bwd: bad argument'),
    ('s2e_instance_norm_bwd', (BAD, P, P, P, P, P, 1, 64, 8, 1, None), -1, 's2e_instance_norm_bwd: bad dtype 7'),
    ('s2e_instance_norm_bwd', (BF16, P, P, P, P, P, 1, 64, 12, 1, None), -3, 's2e_instance_norm_bwd: C=12 not a multiple of 8'),
    ('s2e_instance_norm_bwd', (F32, P, P, P, P, P, 1, 64, 6, 1, None), -3, 's2e_instance_norm_bwd: C=6 not a multiple of 4'),
    ('s2e_loss_reduce', (BF16, 0, None, None, 64, 1.0, P, None), -1, 's2e_loss_reduce: bad argument'),
    ('s2e_loss_reduce', (BF16, 3, P, None, 64, 1.0, P, None), -1, 's2e_loss_reduce: bad argument'),
    ('s2e_loss_reduce', (BAD, 0, P, None, 64, 1.0, P, None), -1, 's2e_loss_reduce: bad dtype 7'),
    ('s2e_loss_reduce', (BAD, 9, P, None, 64, 1.0, P, None), -1, 's2e_loss_reduce: bad dtype 7'),
    ('s2e_loss_reduce', (BF16, 9, P, None, 64, 1.0, P, None), -1, 'loss: bad mode 9'),
    ('s2e_loss_grad', (F32, 0, P, None, 64, 1.0, None, None, 0, None), -1, 's2e_loss_grad: bad argument'),
    ('s2e_loss_grad', (BAD, 0, P, None, 64, 1.0, None, P, 0, None), -1, 's2e_loss_grad: bad dtype 7'),
    ('s2e_loss_grad', (F32, 9, P, None, 64, 1.0, None, P, 0, None), -1, 'loss: bad mode 9'),
    ('s2e_shard_sum', (BF16, P, None, 2, 64, None), -1, 's2e_shard_sum: bad argument'),
    ('s2e_shard_sum', (BAD, P, P, 2, 64, None), -1, 's2e_shard_sum: bad dtype 7'),
    ('s2e_shard_sum', (BF16, P, P, 2, 4, None), -1, 's2e_shard_sum: buffers and the shard size must be 16-byte multiples'),
    ('s2e_shard_sum', (F32, P, P, 2, 6, None), -1, 's2e_shard_sum: buffers and the shard size must be 16-byte multiples'),
    ('s2e_shard_sum', (BAD, P, P, 2, 6, None), -1, 's2e_shard_sum: buffers and the shard size must be 16-byte multiples'),
    ('s2e_fc_head_fwd', (BF16, P, P, None, P, 2, 4, 8, 16, 0.2, None, 0, None), -1, 's2e_fc_head_fwd: bad argument (M=2 N=16)'),
    ('s2e_fc_head_fwd', (BAD, P, P, P, P, 2, 4, 8, 16, 0.2, None, 0, None), -1, 's2e_fc_head_fwd: bad dtype 7'),
    ('s2e_fc_head_fwd', (BAD, P, P, P, P, 2, 4, 8, 32, 0.2, P, 1 << 20, None), -1, 's2e_fc_head_fwd: bad dtype 7'),
    ('s2e_fc_head_fwd', (BF16, P, P, P, P, 2, 4, 8, 64, 0.2, P, 1 << 20, None), -1, 's2e_fc_head_fwd: bad argument (M=2 N=64)'),
    ('s2e_fc_head_fwd', (BF16, P, P, P, P, 2, 256, 64, 16, 0.2, None, 0, None), -3, 's2e_fc_head_fwd: a sample row of 256 x 64 features does not fit the LDS stage'),
    ('s2e_fc_head_bwd', (BF16, P, None, P, P, P, P, 2, 4, 8, 16, 0.2, None), -1, 's2e_fc_head_bwd: bad argument (M=2 N=16)'),
    ('s2e_fc_head_bwd', (BAD, P, P, P, P, P, P, 2, 4, 8, 16, 0.2, None), -1, 's2e_fc_head_bwd: bad dtype 7'),
    ('s2e_pack_conv_weight', (BF16, P, None, None, 64, 64, 3, 3, 64, 0, None), -1, 's2e_pack_conv_weight: bad argument'),
    ('s2e_pack_conv_weight', (BAD, P, P, None, 64, 64, 3, 3, 64, 0, None), -1, 's2e_pack_conv_weight: bad dtype 7'),
    ('s2e_pack_conv_weight', (BAD, P, P, None, 64, 64, 9, 9, 64, 0, None), -1, 's2e_pack_conv_weight: bad dtype 7'),
    ('s2e_pack_conv_weight', (F32, P, P, None, 64, 64, 3, 3, 64, 4, None), -3, 's2e_pack_conv_weight: the plane layout needs bf16, cin_pad == cin and a K dimension that is a multiple of 32'),
    ('s2e_pack_conv_weight', (F32, P, P, None, 64, 60, 3, 3, 60, 2, None), -3, 's2e_pack_conv_weight: a channels-last source needs cin % 8 == 0'),
    ('s2e_pack_conv_weights', (BF16, None, P, 4, 9, None, None), -1, 's2e_pack_conv_weights: bad argument'),
    ('s2e_pack_conv_weights', (BAD, P, P, 4, 9, None, None), -1, 's2e_pack_conv_weights: bad dtype 7'),
    ('s2e_pack_conv_weights', (BAD, P, P, 4, 25, None, None), -1, 's2e_pack_conv_weights: bad dtype 7'),
    ('s2e_conv2d', (BF16, None, P, None, None, None, P, BIG, None, 0, None), -1, 's2e_conv2d: null pointer'),
    ('s2e_conv2d', (BAD, P, P, None, None, None, P, BIG, None, 0, None), -1, 's2e_conv2d: bad dtype 7'),
    ('s2e_conv2d_wgrad', (BF16, P, None, P, None, BIG, None, 0, None), -1, 's2e_conv2d_wgrad: null pointer'),
    ('s2e_conv2d_wgrad', (BAD, P, P, P, None, BIG, None, 0, None), -1, 's2e_conv2d_wgrad: bad dtype 7'),
    ('s2e_spade_conv_modulate', (BF16, P, P, P, P, None, P, 0, P, None, 8, 64, 64, 64, 128, 1, 0, None), -1, 's2e_spade_conv_modulate: null pointer'),
    ('s2e_spade_conv_modulate', (BAD, P, P, P, P, P, P, 0, P, None, 8, 64, 64, 64, 128, 1, 0, None), -1, 's2e_spade_conv_modulate: bad dtype 7'),
    ('s2e_spade_conv_modulate', (BAD, P, P, P, P, P, P, 2, P, None, 8, 64, 64, 64, 128, 1, 0, None), -1, 's2e_spade_conv_modulate: stats, style and bias must be 16-byte aligned (style_ld a multiple of 4)'),
    ('s2e_spade_conv_modulate', (F32, P, P, P, P, P, P, 0, P, None, 8, 64, 64, 64, 24, 1, 0, None), -3, 's2e_spade_conv_modulate: shape N=8 64x64 C=64 nh=24 is not taken by the fused kernel (s2e_spade_conv_modulate_supported); run s2e_conv2d + s2e_modulate_fwd'),
    ('s2e_spade_conv_modulate_sparse', (BF16, P, P, P, P, P, P, 0, P, None, 8, 64, 64, 64, 128, 1, 0, P, None, None), -1, 's2e_spade_conv_modulate_sparse: rect_list / rect_count missing'),
    ('s2e_spade_conv_modulate_sparse', (BAD, P, P, P, P, P, P, 0, P, None, 8, 64, 64, 64, 128, 1, 0, P, P, None), -1, 's2e_spade_conv_modulate: bad dtype 7'),
    ('s2e_openeds_error', (BF16, P, None, 1, 8, 8, P, None), -1, 's2e_openeds_error: bad argument'),
    ('s2e_openeds_error', (BAD, P, P, 1, 8, 8, P, None), -1, 's2e_openeds_error: bad dtype 7'),
    ('s2e_resize_to255', (BF16, None, 1, 8, 8, P, 4, 4, None), -1, 's2e_resize_to255: bad argument'),
    ('s2e_resize_to255', (BAD, P, 1, 8, 8, P, 4, 4, None), -1, 's2e_resize_to255: bad dtype 7'),
    ('s2e_resize_to255', (BAD, P, 1, 8, 8, P, 70000, 4, None), -3, 's2e_resize_to255: grid too large'),
    ('s2e_sidebyside_u8', (BF16, None, P, 1, P, P, 1, 8, 8, 8, 8, 4, 4, 20, 80, P, P, P, None), -1, 's2e_sidebyside_u8: bad argument fake (null)'),
    ('s2e_sidebyside_u8', (BAD, P, P, 1, P, P, 1, 8, 8, 8, 8, 4, 4, 20, 80, P, P, P, None), -1, 's2e_sidebyside_u8: bad argument fake_dtype'),
    ('s2e_sidebyside_u8', (BAD, None, P, 1, P, P, 1, 8, 8, 8, 8, 4, 4, 20, 80, P, P, P, None), -1, 's2e_sidebyside_u8: bad argument fake_dtype'),
]
# the host-only size queries, one bf16 and one fp32 shape each (and a C that breaks the vector-width rule: 0)
HOST_QUERY_TABLE = [
    ('s2e_in_stats_workspace_bytes', (BF16, 2, 4096, 64), 10240),
    ('s2e_in_stats_workspace_bytes', (F32, 2, 4096, 64), 18432),
    ('s2e_in_stats_workspace_bytes', (BF16, 2, 4096, 12), 0),
    ('s2e_modulate_bwd_workspace_bytes', (BF16, 2, 4096, 64), 22528),
    ('s2e_modulate_bwd_workspace_bytes', (F32, 2, 4096, 64), 38912),
    ('s2e_modulate_bwd_workspace_bytes', (BF16, 2, 4096, 12), 0),
]


def test_dtype_entry_points_reject_bad_calls_before_any_launch():
    """The return code and the message of an invalid call are the library's behaviour, including which check wins when several
    fail.  Host-only: with a GPU visible the test skips itself, so that a dummy pointer can never reach a kernel."""
    if torch.cuda.is_available():
        pytest.skip('dummy pointers: host-only by construction')
    from seg2eye_amd import _lib
    L = _lib.lib()
    assert (_lib.S2E_BF16, _lib.S2E_F32, _lib.NORM_SPADE_STYLE, _lib.NORM_ACCUMULATE_DX) == (BF16, F32, SP, ACC)
    assert len({name for name, _, _, _ in HOST_ERROR_TABLE}) == 35
    got = []
    for name, args, _, _ in HOST_ERROR_TABLE:
        rc = getattr(L, name)(*[ctypes.byref(_lib.ConvDesc(*a[1:])) if a is BIG else a for a in args])
        got.append((name, args, rc, L.s2e_last_error().decode() if rc else ''))
    wrong = [(g, w) for g, w in zip(got, HOST_ERROR_TABLE) if g != w]
    assert not wrong, wrong
    for name, args, want in HOST_QUERY_TABLE:
        assert getattr(L, name)(*args) == want, (name, args)


# ------------------------------------------------------------------------------------------------ the binding against the header
# the 11 job structures of include/seg2eye_hip.h and the ctypes classes that mirror them
STRUCTS = {'s2e_conv_desc': 'ConvDesc', 's2e_pack_job': 'PackJob', 's2e_wgrad_multi_job': 'WgradMultiJob', 's2e_sn_layer': 'SnLayer',
           's2e_sngrad_job': 'SnGradJob', 's2e_grad_job': 'GradJob', 's2e_wgrad_c8_job': 'WgradC8Job', 's2e_wgrad_batch_job': 'WgradBatchJob',
           's2e_spade_uni_job': 'SpadeUniJob', 's2e_class_table_job': 'ClassTableJob', 's2e_label_conv_job': 'LabelConvJob'}
_SCALARS = ('int', 'long', 'size_t', 'float', 'double')


def _header_text():
    text = open(os.path.join(ROOT, 'include', 'seg2eye_hip.h')).read()
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text, flags=re.S))


def _c_class(ctype, returned=False):
    """The class of a C type spelled as in the header, stars included ('const float*'): a scalar's name, 'ptr', 'conv_desc*',
    'conv_desc' (nested) or, for a returned const char*, 'text'."""
    words = [w for w in ctype.replace('*', ' ').split() if w not in ('const', 'struct')]
    if '*' in ctype:
        assert ctype.count('*') == 1, ctype
        return 'text' if (returned and words == ['char']) else 'conv_desc*' if words == ['s2e_conv_desc'] else 'ptr'
    if words == ['s2e_conv_desc']:
        return 'conv_desc'
    assert len(words) == 1 and words[0] in _SCALARS, 'a type this test has no class for: %r' % ctype
    return words[0]


def _declarators(decl):
    """'const float *a, *b' / 'int N, Hi' / 'const void* x' -> [(class, name), ...]"""
    first, *more = decl.split(',')
    m = re.fullmatch(r'\s*(.*?)(\w+)\s*', first)
    assert m and m.group(1).strip(), decl
    base = m.group(1).replace('*', '')
    return [(_c_class(m.group(1)), m.group(2))] + [(_c_class(base + '*' * d.count('*')), d.replace('*', '').strip()) for d in more]


def _ctypes_class(t):
    from seg2eye_amd import _lib
    table = {ctypes.c_int: 'int', ctypes.c_long: 'long', ctypes.c_size_t: 'size_t', ctypes.c_float: 'float', ctypes.c_double: 'double',
             ctypes.c_void_p: 'ptr', _lib.ConvDesc: 'conv_desc', ctypes.POINTER(_lib.ConvDesc): 'conv_desc*'}
    assert ctypes.c_size_t is not ctypes.c_long                  # (distinct classes here: the comparison below tells them apart)
    return table[t]


def test_mirrored_constants_are_the_headers():
    """The fused SPADE launch's flag bits (and the replica count of the uniform sums) in _lib against the header's #defines."""
    from seg2eye_amd import _lib
    defs = {k: int(v) for k, v in re.findall(r'(?m)^#define\s+S2E_(\w+)\s+(\d+)\s*$', _header_text())}
    for name in ('SPADE_ANY_TILES', 'SPADE_DENSE', 'SPADE_ANY_RECTS', 'SPADE_X_HALF', 'UNI_REPLICAS'):
        assert getattr(_lib, name) == defs[name], name
    assert (_lib.SPADE_ANY_TILES, _lib.SPADE_DENSE, _lib.SPADE_ANY_RECTS, _lib.SPADE_X_HALF) == (1, 2, 4, 8)


def test_binding_agrees_with_the_header_in_arguments_return_types_and_structures():
    """_lib.SIGNATURES and the ctypes structures are a second copy of include/seg2eye_hip.h: compare them position by position --
    argument count, the class of every argument, the return class against the entry's kind, and every field of the job structures."""
    from seg2eye_amd import _lib
    text = _header_text()
    decls = re.findall(r'(?m)^\s*((?:const\s+)?\w+)\s*(\*?)\s*(s2e_\w+)\s*\(([^)]*)\)\s*;', text)
    assert len(decls) >= 100 and sorted(n for _, _, n, _ in decls) == sorted(_lib.SIGNATURES), len(decls)
    returns = {_lib.STATUS: 'int', _lib.VALUE: 'int', _lib.COUNT: 'long', _lib.SIZE: 'size_t', _lib.TEXT: 'text'}
    wrong = []
    for rtype, rstar, name, params in decls:
        kind, argtypes = _lib.SIGNATURES[name]
        if _c_class(rtype + rstar, returned=True) != returns[kind]:
            wrong.append((name, 'returns', rtype + rstar, kind))
        params = [] if params.strip() in ('', 'void') else [p.strip() for p in params.split(',')]
        if len(params) != len(argtypes):
            wrong.append((name, 'argument count', len(params), len(argtypes)))
            continue
        for i, (p, t) in enumerate(zip(params, argtypes)):
            (want, _), = _declarators(p)
            got = _ctypes_class(t)
            if not (got == want or (got == 'ptr' and want == 'conv_desc*')):
                wrong.append((name, 'argument %d' % i, p, got))
    assert not wrong, wrong
    structs = re.findall(r'typedef\s+struct\s*\w*\s*\{([^}]*)\}\s*(\w+)\s*;', text)
    assert len(structs) == 11 and sorted(n for _, n in structs) == sorted(STRUCTS), [n for _, n in structs]
    for body, name in structs:
        want = [f for decl in body.split(';') if decl.strip() for f in _declarators(decl.strip())]
        got = [(_ctypes_class(t), n) for n, t in getattr(_lib, STRUCTS[name])._fields_]
        assert got == want, (name, [(g, w) for g, w in zip(got, want) if g != w], len(got), len(want))


def test_checked_handle_raises_where_the_raw_one_returns_a_code():
    from seg2eye_amd import _lib
    raw = _lib.lib()
    assert raw.s2e_colsum(_lib.S2E_BF16, None, 10, 8, None, None) == -1
    with pytest.raises(_lib.Seg2EyeHipError) as e:
        _lib.check(-1, 's2e_colsum')
    with pytest.raises(_lib.Seg2EyeHipError) as e2:
        _lib.call.s2e_colsum(_lib.S2E_BF16, None, 10, 8, None, None)
    assert str(e2.value) == str(e.value) and str(e2.value).startswith('s2e_colsum failed (-1): ')
    assert raw.s2e_last_error().decode() in str(e2.value) and 's2e_colsum: bad argument' in str(e2.value)
    # a COUNT planner: the code comes back as the count (no error text is set): name and code only
    jobs = (_lib.LabelConvJob * 1)()
    jobs[0].weight, jobs[0].h, jobs[0].w, jobs[0].cout = 64, 16, 16, 129          # (cout > 128: S2E_ERR_ARG; the weight is never read)
    args = (_lib.S2E_BF16, ctypes.byref(jobs), 1, 2, None)
    assert raw.s2e_label_conv_block_map(*args) == -1
    with pytest.raises(_lib.Seg2EyeHipError) as e3:
        _lib.call.s2e_label_conv_block_map(*args)
    assert str(e3.value) == 's2e_label_conv_block_map failed (-1)'
    jobs[0].cout = 128
    assert _lib.call.s2e_label_conv_block_map(*args) == raw.s2e_label_conv_block_map(*args) > 0
    # the checked handle is bound once and then served from its instance dictionary; lib() stays raw
    assert _lib.call.__dict__['s2e_colsum'] is _lib.call.s2e_colsum and _lib.call.s2e_colsum is not raw.s2e_colsum
    assert _lib.call.s2e_sn_block_shape(0, None, None) == 0 and _lib.call.s2e_version() == raw.s2e_version()


def test_dtype_code_takes_tensors_and_dtypes_and_refuses_the_rest_first():
    from seg2eye_amd import _lib, ops
    from seg2eye_amd.packing import PackPlan
    assert ops._dt(torch.bfloat16) == ops._dt(torch.zeros(1, dtype=torch.bfloat16)) == _lib.S2E_BF16
    assert ops._dt(torch.float32) == ops._dt(torch.zeros(1)) == _lib.S2E_F32
    for bad in (torch.float16, torch.float64):
        with pytest.raises(TypeError, match='bf16 or fp32'):
            ops._dt(bad)
        with pytest.raises(TypeError, match='bf16 or fp32'):
            ops._dt(torch.zeros(1, dtype=bad))
    w = torch.zeros(8, 8, 3, 3)                                  # a CPU tensor: the "GPU only" error would come next
    for plane in (False, True):
        with pytest.raises(TypeError, match='bf16 or fp32'):
            ops.pack_weight(w, torch.float16, plane=plane)
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        ops.pack_weight(w, torch.bfloat16)
    with pytest.raises(TypeError, match='bf16 or fp32'):
        PackPlan().record(w, torch.float16, 8, False, None)
    with pytest.raises(TypeError, match='bf16 or fp32'):
        ops.label_rects(torch.zeros(1, 16, 16, dtype=torch.uint8), 16, 16, torch.float16, 64, 128)
    with pytest.raises(TypeError, match='bf16 or fp32'):
        ops.SpadePrepass.table(torch.float16, w, w, w, w, 4, 128, 64, False)


def test_profiler_off_is_a_plain_call():
    from seg2eye_amd.ops import LaunchProfiler

    def boom():
        raise AssertionError('evaluated with no profiler installed')
    assert not LaunchProfiler.active()
    assert LaunchProfiler.run('x', 1.0, lambda a, b: (a, b), (1, 2), tag=boom, nbytes=boom) == (1, 2)
    assert LaunchProfiler.run(boom, 1.0, max, (1, 2), executed=3.0) == 2
