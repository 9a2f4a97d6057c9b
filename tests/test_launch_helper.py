"""ops.launch: the one call of a library entry point.  A stub stands in for the shared object, so the contract of the helper --
pointer conversion by the declared argument types, NULL, the stream, arity, the return code, the byte accounting and the
timing scope -- is checked without a device."""
import pytest
import torch

from latentfusion_amd import _lib, ops

STREAM = 0x5EED


class _StubLib:
    """`lf_*` attributes record their arguments and return `rc`."""

    def __init__(self, rc=0):
        self.rc, self.calls = rc, []

    def __getattr__(self, name):
        if not name.startswith('lf_'):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return self.rc
        return fn


@pytest.fixture
def stub(monkeypatch):
    lib = _StubLib()
    monkeypatch.setattr(_lib, '_lib', lib)
    monkeypatch.setattr(ops, '_stream', lambda: STREAM)
    monkeypatch.setattr(ops, 'KERNEL_TIMER', None)
    monkeypatch.setattr(_lib, 'BYTE_LOG', None)
    return lib


def _wino_args(x, upack, y, bias=None, norm=None, py=None, pn=None, amax=None):
    """The 17 arguments of lf_conv3d_c16_wino before the stream (five of the pointers optional)."""
    return (x, upack, bias, y, norm, 1, 4, 4, 4, 0.125, 3, 0.2, 1e-8, py, pn, 0, amax)


def test_signatures_used_here():
    assert len(_lib.SIGNATURES['lf_conv3d_c16_wino'][1]) == 18
    assert len(_lib.SIGNATURES['lf_pixelnorm_fwd'][1]) == 7


def test_tensor_parameter_none_and_scalars(stub):
    x, y = torch.zeros(16), torch.zeros(16)
    upack = torch.nn.Parameter(torch.zeros(8))
    ops.launch('lf_conv3d_c16_wino', *_wino_args(x, upack, y))
    (name, args), = stub.calls
    assert name == 'lf_conv3d_c16_wino'
    assert args[0] == x.data_ptr() and type(args[0]) is int                 # tensor -> data_ptr()
    assert args[1] == upack.data_ptr() and type(args[1]) is int             # nn.Parameter -> data_ptr()
    assert args[3] == y.data_ptr()
    assert args[2] is None and args[4] is None and args[13] is None and args[14] is None and args[16] is None   # None -> NULL
    assert args[5:13] == (1, 4, 4, 4, 0.125, 3, 0.2, 1e-8) and args[15] == 0                                     # untouched
    assert [type(v) for v in args[5:13]] == [int, int, int, int, float, int, float, float]
    assert len(args) == 18 and args[-1] == STREAM                           # the stream goes last


def test_raw_int_pointer_is_passed_as_it_is(stub):
    x = torch.zeros(16)
    ops.launch('lf_pixelnorm_fwd', x.data_ptr() + 8, 1234, None, 4, 4, 1e-8)
    assert stub.calls[0][1] == (x.data_ptr() + 8, 1234, None, 4, 4, 1e-8, STREAM)


@pytest.mark.parametrize('n', [16, 18])
def test_wrong_arity_is_a_type_error_naming_the_entry_point(stub, n):
    x = torch.zeros(16)
    args = (_wino_args(x, x, x) + (0,))[:n]
    with pytest.raises(TypeError, match='lf_conv3d_c16_wino'):
        ops.launch('lf_conv3d_c16_wino', *args)
    assert stub.calls == []


def test_tensor_at_an_int_position_is_not_converted(stub):
    x, rows = torch.zeros(16), torch.tensor(4)
    ops.launch('lf_pixelnorm_fwd', x, x, x, rows, 4, 1e-8)          # rows is c_long: ctypes, not the helper, judges it
    assert stub.calls[0][1][3] is rows


def test_experimental_entry_points_are_known(stub):
    x = torch.zeros(16)
    ops.launch('lf_resample3d_bwd_vol', x, x, 0, x, 1, 1, 2, 2, 2, 16)
    assert stub.calls[0][1][:2] == (x.data_ptr(), x.data_ptr()) and stub.calls[0][1][-1] == STREAM


def test_return_code_raises_with_the_name(stub):
    stub.rc = -2
    x = torch.zeros(16)
    with pytest.raises(_lib.LFHipError, match='lf_pixelnorm_fwd'):
        ops.launch('lf_pixelnorm_fwd', x, x, x, 4, 4, 1e-8)


def test_byte_accounting(stub, monkeypatch):
    monkeypatch.setattr(_lib, 'BYTE_LOG', {})
    monkeypatch.setattr(_lib, '_PENDING', [0])
    x, y, upack = torch.zeros(64), torch.zeros(64), torch.zeros(32, dtype=torch.float16)
    bias = torch.zeros(16, 1).expand(16, 100)                      # an expanded view: 1600 elements over 64 bytes of storage
    scratch = torch.zeros(1000)
    ops.launch('lf_conv3d_c16_wino', *_wino_args(x, upack, y, bias=bias, amax=scratch.data_ptr()))
    assert _lib.BYTE_LOG == {'lf_conv3d_c16_wino': [1, 256 + 64 + 256 + 64]}     # the raw-int pointer is not counted
    ops.launch('lf_pixelnorm_fwd', y, y, x, 4, 16, 1e-8)           # in place: y is counted once per argument
    assert _lib.BYTE_LOG['lf_pixelnorm_fwd'] == [1, 3 * 256]
    ops.launch('lf_pixelnorm_fwd', y.data_ptr(), y.data_ptr(), None, 4, 16, 1e-8)
    assert _lib.BYTE_LOG['lf_pixelnorm_fwd'] == [2, 3 * 256]
    assert _lib._PENDING == [0]


def test_byte_accounting_equals_the_ptr_form(stub, monkeypatch):
    """The same launch spelled with ops._ptr and _lib.check, as the wrappers used to: the same entry."""
    x, y, n = torch.zeros(64), torch.zeros(48), torch.zeros(4)
    monkeypatch.setattr(_lib, 'BYTE_LOG', {})
    _lib.check(_lib.lib().lf_pixelnorm_fwd(ops._ptr(x), ops._ptr(y), ops._ptr(n), 4, 16, 1e-8, ops._stream()), 'lf_pixelnorm_fwd')
    old = _lib.BYTE_LOG
    monkeypatch.setattr(_lib, 'BYTE_LOG', {})
    ops.launch('lf_pixelnorm_fwd', x, y, n, 4, 16, 1e-8)
    assert _lib.BYTE_LOG == old and stub.calls[0] == stub.calls[1]


class _FakeEvent:
    made = []

    def __init__(self, enable_timing=False):
        _FakeEvent.made.append(self)
        self.records = 0

    def record(self):
        self.records += 1


@pytest.fixture
def events(monkeypatch):
    monkeypatch.setattr(_FakeEvent, 'made', [])
    monkeypatch.setattr(torch.cuda, 'Event', _FakeEvent)
    return _FakeEvent.made


def test_no_timer_no_events(stub, events):
    x = torch.zeros(16)
    ops.launch('lf_pixelnorm_fwd', x, x, x, 4, 4, 1e-8, tag='pixelnorm', detail='4x4')
    ops.launch('lf_pixelnorm_fwd', x, x, x, 4, 4, 1e-8)
    assert events == [] and len(stub.calls) == 2


def test_tag_and_detail_reach_the_timer(stub, events, monkeypatch):
    timer = []
    monkeypatch.setattr(ops, 'KERNEL_TIMER', timer)
    monkeypatch.setattr(ops, 'KERNEL_TIMER_TAGS', None)
    x = torch.zeros(16)
    ops.launch('lf_pixelnorm_fwd', x, x, x, 4, 4, 1e-8)                                  # untagged: not timed
    assert timer == [] and events == []
    ops.launch('lf_pixelnorm_fwd', x, x, x, 4, 4, 1e-8, tag='conv3d_c16_wino', detail='fwd:8:io0')
    (tag, e0, e1), = timer
    assert tag == 'conv3d_c16_wino' and tag.detail == 'fwd:8:io0'
    assert events == [e0, e1] and e0.records == 1 and e1.records == 1
    monkeypatch.setattr(ops, 'KERNEL_TIMER_TAGS', {'other'})                              # the tag filter of _timed applies
    ops.launch('lf_pixelnorm_fwd', x, x, x, 4, 4, 1e-8, tag='conv3d_c16_wino')
    assert len(timer) == 1 and len(events) == 2 and len(stub.calls) == 3
