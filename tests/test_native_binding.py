"""The binding of the native libraries without a GPU: the one loader and the one launch path of stabstitch2_amd/_hip.py, the two
return-code policies, and that no library's header knows of a library added after it.  A stub stands in for a loaded library: its
attributes are Python callables that record the call and return a chosen code.
    python -m pytest tests/test_native_binding.py"""
import re

import pytest

import abi_surface as A
from stabstitch2_amd import _hip

MODULES = A.modules()
SIDE = MODULES[1:]
IDS = [m.__name__.split('.')[-1] for m in MODULES]


class Stub:
    def __init__(self, code=0):
        self.code, self.calls = code, []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return self.code
        return entry

    def ss_error_string(self, code):
        return b'bad argument' if code == -1 else b'other'


def devptr(dev):
    p = _hip.DevPtr(4096)
    p.dev = dev
    return p


def test_the_list_names_the_five_modules_and_their_prefixes():
    assert _hip.LIBRARIES == ('_hip', '_blend', '_seam', '_mbwarp', '_surfaces') and MODULES[0] is _hip
    assert [m.PREFIX for m in MODULES] == ['ss_', 'ssb_', 'ssm_', 'ssw_', 'ssf_']
    assert [m.API for m in MODULES] == ['SS_API', 'SSB_API', 'SSM_API', 'SSW_API', 'SSF_API']
    for m in MODULES:
        assert m.LIB_PATH.endswith('lib%s.so' % m.HEADER[:-2]) and all(name.startswith(m.PREFIX) for name in m.SIGNATURES)
        assert m.ERR_ARG == -1


# ------------------------------------------------------------------------------------------------ the headers
@pytest.mark.parametrize('module', MODULES, ids=IDS)
def test_a_header_declares_its_own_prefix_and_no_earlier_header_knows_of_it(module):
    """Every name a header declares under its macro carries its own prefix, whichever library it is.  A later library may build on
    the earlier ones and say so (stabstitch_mbwarp.h names entry points of all three before it); an earlier one neither declares nor
    mentions a symbol with the prefix of a later one, nor its header: (hip | ssb_), (hip, blend | ssm_), (hip, blend, seam | ssw_),
    (hip, blend, seam, mbwarp | ssf_)."""
    names = re.findall(r'^%s\b[^;(]*?\b(\w+)\s*\(' % module.API, A.header(module), re.M)       # (a line that begins with the macro)
    assert len(names) == len(module.SIGNATURES) and all(n.startswith(module.PREFIX) for n in names), names
    before = A.headers_before(module)
    assert len(before) == MODULES.index(module)
    pattern = '%s|%s' % (module.PREFIX, re.escape(module.HEADER[len('stabstitch_'):]))        # e.g. ssm_|seam\.h
    for other, text in before.items():
        assert not re.search(pattern, text), (other, pattern)


# ------------------------------------------------------------------------------------------------ the loader
def test_load_of_a_missing_library_says_how_to_build_it(tmp_path):
    path = str(tmp_path / 'libstabstitch_absent.so')
    with pytest.raises(ImportError) as e:
        _hip.load(path, {})
    assert path in str(e.value) and '%s not found' % path in str(e.value)
    assert 'python -c "import __graft_entry__ as g; g.build()"' in str(e.value) and 'stabstitch2_amd/csrc/build.sh' in str(e.value)
    assert 'There is no CPU fallback' in str(e.value)


# ------------------------------------------------------------------------------------------------ the launch path
@pytest.mark.parametrize('module', SIDE, ids=IDS[1:])
def test_a_side_call_refuses_before_the_entry_point(module, monkeypatch):
    stub = Stub()
    monkeypatch.setattr(module, '_lib', stub)
    name = sorted(module.SIGNATURES)[0]
    with pytest.raises(_hip.HipError, match='^%s needs device tensors; there is no CPU path$' % name):
        module.call(name, 1, 2, _hip.stream())
    with pytest.raises(_hip.HipError, match=r'^%s: tensors of one launch live on different GPUs \(cuda:0 and cuda:1\)$' % name):
        module.call(name, devptr(0), 3, devptr(1), _hip.stream())
    assert stub.calls == []


def test_the_main_call_takes_host_arguments_and_maps_every_code_to_hip_error(monkeypatch):
    stub = Stub()
    monkeypatch.setattr(_hip, '_lib', stub)
    assert _hip.call('ss_conv_workspace_need', 1, 2) is None and stub.calls == [('ss_conv_workspace_need', (1, 2))]
    stub.code = -1
    with pytest.raises(_hip.HipError, match=r'^ss_fill_f32 failed: bad argument \(-1\)$') as e:
        _hip.call('ss_fill_f32', None, 0.0, 0)
    assert e.value.code == -1 and not isinstance(e.value, ValueError) and len(stub.calls) == 2
    with pytest.raises(_hip.HipError, match=r'^ss_add_mul: tensors of one launch live on different GPUs \(cuda:1 and cuda:0\)$'):
        _hip.call('ss_add_mul', devptr(1), devptr(0))
    assert len(stub.calls) == 2


# ------------------------------------------------------------------------------------------------ the return codes
def test_return_codes_of_the_side_libraries():
    assert _hip.check_side(0, 'ssf_nv12_to_bgr') is None
    with pytest.raises(ValueError, match='^ssf_nv12_to_bgr refused its arguments$') as e:
        _hip.check_side(-1, 'ssf_nv12_to_bgr')
    assert not isinstance(e.value, _hip.HipError)
    with pytest.raises(_hip.HipError, match=r'^ssm_multiband_seam failed: launch error \(-2\)$') as e:
        _hip.check_side(-2, 'ssm_multiband_seam')
    assert e.value.code == -2
