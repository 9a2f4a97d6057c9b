"""CPU tests of the host side of lf_rows_gemm_epi (the ranking path's factor projection as one in-tree MFMA launch): the
documented weight layout of ops.pack_rows_gemm, lf_rows_gemm_cout_padded, and the argument rules of `proj_kernel` in the
engine and the estimators as far as they are decidable without a GPU.  No kernel is launched here."""
import pytest
import torch


def _unpack(wpack, cout):
    """The layout documented at the prototype (include/lf_hip.h): wpack[co][k] = W[co][k], [CoutP][K] row-major."""
    return wpack[:cout]


@pytest.mark.parametrize('cout', [16, 100, 256])
@pytest.mark.parametrize('k', [4, 20, 4096])
def test_pack_rows_gemm_round_trip(cout, k):
    from latentfusion_amd import _lib, ops
    g = torch.Generator().manual_seed(cout * 10007 + k)
    w = torch.randn(cout, k, generator=g)
    wpack = ops.pack_rows_gemm(w)
    coutp = _lib.lib().lf_rows_gemm_cout_padded(cout)
    assert wpack.dtype == torch.float32 and wpack.is_contiguous() and tuple(wpack.shape) == (coutp, k)
    assert torch.equal(_unpack(wpack, cout), w)
    assert wpack[cout:].numel() == (coutp - cout) * k and not wpack[cout:].any()        # padded rows exactly zero
    assert not w.requires_grad and not wpack.requires_grad
    wp = torch.nn.Parameter(w.clone())
    assert not ops.pack_rows_gemm(wp).requires_grad and torch.equal(ops.pack_rows_gemm(wp), wpack)


def test_cout_padded_agrees_with_the_packer_and_the_domain():
    from latentfusion_amd import _lib, ops
    L = _lib.lib()
    want = {16: 16, 20: 32, 32: 32, 36: 64, 64: 64, 68: 128, 100: 128, 128: 128, 132: 192, 192: 192, 196: 256, 256: 256}
    for cout, coutp in want.items():
        assert L.lf_rows_gemm_cout_padded(cout) == coutp
        assert ops.pack_rows_gemm(torch.zeros(cout, 8)).shape[0] == coutp
    for cout in range(16, 257, 4):
        p = L.lf_rows_gemm_cout_padded(cout)
        assert p >= cout and p % 16 == 0 and p in (16, 32, 64, 128, 192, 256)
    for bad in (0, -4, 257, 260, 1024):
        assert L.lf_rows_gemm_cout_padded(bad) == 0
    for cout, k in ((260, 8), (18, 8), (12, 8), (16, 6), (16, 0)):
        with pytest.raises(ValueError):
            ops.pack_rows_gemm(torch.zeros(cout, k))


def test_select_proj_kernel_rules():
    from latentfusion_amd.engine import PROJ_KERNELS, RenderLoopEngine, select_proj_kernel
    assert PROJ_KERNELS == ('library', 'mfma')
    assert RenderLoopEngine.PROJ_KERNEL == 'library' and RenderLoopEngine.PROJ_GEMM is True       # the default does not change
    assert select_proj_kernel(None, 'library', 4096, 256) == 'library'
    assert select_proj_kernel(None, 'mfma', 4096, 256) == 'mfma'
    assert select_proj_kernel('mfma', 'library', 4096, 256) == 'mfma'
    assert select_proj_kernel('mfma', 'library', 16 * 16, 16) == 'mfma'
    assert select_proj_kernel('library', 'mfma', 16 * 512, 512) == 'library'       # the library path has no such limit
    assert select_proj_kernel('library', 'library', None, None) == 'library'       # ('sum' projection: the option is idle)
    for bad in ('hipblaslt', 'MFMA', '', True):
        with pytest.raises(ValueError):
            select_proj_kernel(bad, 'library', 4096, 256)
    # outside the kernel's domain: refused, never a silent fall-back to the library
    for K, cout in ((16 * 512, 512), (4096, 260), (4096, 18), (4096, 12), (6, 16), (None, None)):
        with pytest.raises(NotImplementedError):
            select_proj_kernel('mfma', 'library', K, cout)
        with pytest.raises(NotImplementedError):
            select_proj_kernel(None, 'mfma', K, cout)


def test_engines_take_proj_kernel():
    import inspect
    from latentfusion_amd.engine import RenderLoopEngine
    from latentfusion_amd.engine_multi import MultiTargetEngine
    from latentfusion_amd.experimental import RenderLoopEngineX
    for cls in (RenderLoopEngine, MultiTargetEngine, RenderLoopEngineX):
        p = inspect.signature(cls.__init__).parameters
        assert 'proj_kernel' in p and p['proj_kernel'].default is None, cls


class _Stub:
    device = 'cpu'


def test_estimators_take_proj_kernel():
    from latentfusion_amd.pose import estimation
    kw = dict(model=_Stub(), ranking_size=4, loss_weights={'depth': 1.0})
    assert estimation.PoseEstimator(**kw).proj_kernel is None
    for v in ('library', 'mfma', None):
        assert estimation.PoseEstimator(proj_kernel=v, **kw).proj_kernel == v
        ce = estimation.CrossEntropyPoseEstimator(num_samples=8, num_elites=2, num_iters=1, num_gmm_components=2,
                                                  learning_rate=0.9, proj_kernel=v, **kw)
        assert ce.proj_kernel == v
        gr = estimation.GradientPoseEstimator(learning_rate=0.01, num_samples=4, num_iters=1, converge_threshold=1e-6,
                                              converge_patience=10, proj_kernel=v, **kw)
        assert gr.proj_kernel == v
    with pytest.raises(ValueError):
        estimation.PoseEstimator(proj_kernel='hipblaslt', **kw)
    # on the host there is no engine (the volume is not on a device): the option is carried, nothing is built
    est = estimation.PoseEstimator(proj_kernel='mfma', **kw)
    assert est._engine_for(torch.zeros(1, 1, 4, 2, 2, 2), None) is None
