"""Frame::ComputeImagePyramid (reference src/Frame.cpp:74-81: cv::pyrDown per level) on packed device pyramids:
the one-launch-per-pyramid kernel (band buffers in LDS) and the one-launch-per-level kernels against the CPU
oracle, byte for byte, on batches — several band heights, 3..5 levels, odd heights, and shapes that are not
eligible for the fused kernel (they must fall back, with the same bytes)."""
import ctypes as C

import numpy as np
import pytest

from dsdtm_amd import capi
from tests import pyrdown_cases as PC

pytestmark = pytest.mark.gpu


def _run(gpu_ctx, imgs, levels, env):
    import torch
    n, h, w = imgs.shape
    ws, hs, ss, offs, nbytes = capi.pyramid_layout(w, h, levels)
    pitch = (nbytes + 255) // 256 * 256
    host = np.zeros((n, pitch), np.uint8)
    host[:, :w * h] = imgs.reshape(n, -1)
    # poison the levels that are to be written
    host[:, offs[1]:nbytes] = 0xA5
    dev = torch.from_numpy(host).to("cuda:0")
    wa, ha, sa = (C.c_int * levels)(*ws), (C.c_int * levels)(*hs), (C.c_int * levels)(*ss)
    oa = (C.c_size_t * levels)(*offs)
    import contextlib
    with (capi.debug_options(**env) if env else contextlib.nullcontext()):
        st = torch.cuda.current_stream()
        gpu_ctx.check(gpu_ctx.lib.dsdtm_pyrdown_batch_device(gpu_ctx.handle, dev.data_ptr(), pitch, n, levels, wa, ha, sa, oa,
                                                            st.cuda_stream))
        torch.cuda.synchronize()
    out = dev.cpu().numpy()
    return [[out[i, offs[l]:offs[l] + ws[l] * hs[l]].reshape(hs[l], ws[l]) for l in range(levels)] for i in range(n)], \
        out[:, nbytes:]


@pytest.mark.parametrize("shape,levels,n", [((480, 640), 4, 5), ((480, 640), 5, 3), ((480, 640), 3, 2),
                                            ((250, 640), 4, 3), ((960, 1280), 4, 2), ((37, 64), 3, 4),
                                            ((241, 323), 4, 2), ((60, 80), 4, 3), ((120, 160), 3, 40)])
def test_batched_pyramids_match_the_oracle(gpu_ctx_each, oracle, shape, levels, n):
    gpu_ctx = gpu_ctx_each                                 # the release library's own choice of kernel; then every variant on the diagnostic one
    rng = np.random.default_rng(shape[0] * 7 + levels)
    imgs = rng.integers(0, 256, (n,) + shape, dtype=np.uint8)
    imgs[0, :, :] = 255                                    # saturation: (sum + 128) >> 8 must stay 255
    want = []
    for i in range(n):
        pyr = [imgs[i]]
        for _ in range(1, levels):
            pyr.append(oracle.pyrdown(pyr[-1]))
        want.append(pyr)
    ref_tail = None
    # band heights: automatic, the smallest, one that does not divide the coarsest level, the whole level
    F = {"pyr_fused": 2}                                  # the fused kernel wherever the shape allows it
    envs = ({}, F, dict(F, pyr_band=2), dict(F, pyr_band=7), dict(F, pyr_band=100000), {"pyr_fused": 0}) if gpu_ctx.diag else ({},)
    for env in envs:
        got, tail = _run(gpu_ctx, imgs, levels, env)
        for i in range(n):
            for l in range(levels):
                assert np.array_equal(got[i][l], want[i][l]), f"{env}: image {i} level {l}"
        # nothing is written behind the last level
        assert not tail.any(), f"{env}: bytes behind the pyramid were written"


# ---- the caller's layouts (tests/pyrdown_cases.py) ----------------------------------------------------------------------
@pytest.mark.parametrize("name", PC.NAMES)
def test_caller_layouts_match_the_oracle_and_leave_every_other_byte(gpu_ctx_each, oracle, name):
    """Row padding, offsets that are 4 and 1 modulo 16, levels out of order, a source level that ends at the pitch, every
    width class of the strip code, heights from 1 row on: levels 1.. equal the oracle's chain byte for byte, and every byte
    the call may not write — level 0, padding (poisoned, with 0x00 / 0xFF next to level 0's rows), the gaps between the
    levels, the bytes behind the last level and behind the last image — is what was uploaded. The release library's own
    choice of kernel (128x288_L5_packed: pyrdown_fused_kernel<4> with 256 threads); then every variant on the diagnostic
    one. That no load goes behind pyr + n * pitch (the `reversed` and `mid_last` layouts) rests on the code, not on this
    run: the buffer has spare bytes behind the last image."""
    import contextlib
    import torch
    gpu_ctx = gpu_ctx_each
    b = PC.build(name)
    c = b.case
    want = PC.expected(oracle, name)
    wa, ha, sa = (C.c_int * c.levels)(*b.ws), (C.c_int * c.levels)(*b.hs), (C.c_int * c.levels)(*b.strides)
    oa = (C.c_size_t * c.levels)(*b.offs)
    F = {"pyr_fused": 2}
    envs = ({}, F, dict(F, pyr_band=2), dict(F, pyr_band=7), dict(F, pyr_band=100000), {"pyr_fused": 0}) if gpu_ctx.diag else ({},)
    for env in envs:
        dev = torch.from_numpy(b.host.copy()).to("cuda:0")
        assert dev.data_ptr() % 16 == 0 and dev.numel() == b.base_shift + c.n * b.pitch + PC.SPARE
        with (capi.debug_options(**env) if env else contextlib.nullcontext()):
            st = torch.cuda.current_stream()
            gpu_ctx.check(gpu_ctx.lib.dsdtm_pyrdown_batch_device(gpu_ctx.handle, dev.data_ptr() + b.base_shift, b.pitch, c.n, c.levels,
                                                                wa, ha, sa, oa, st.cuda_stream))
            torch.cuda.synchronize()
        got = dev.cpu().numpy()
        for i in range(c.n):
            for l in range(1, c.levels):
                assert np.array_equal(b.level(got, i, l), b.level(want, i, l)), f"{env}: image {i} level {l}"
        changed = np.nonzero((got != b.host) & ~b.writable)[0]
        assert changed.size == 0, f"{env}: {changed.size} bytes outside levels 1.. were written, the first at {changed[0]}"
