"""The surface of a native library, checked one way for every binding module of stabstitch2_amd._hip.LIBRARIES: what its header
declares == its ctypes table == what the built library exports.  A plain helper module (imported like sweep_inputs): the tests keep
what is their own -- the names, the #define comparisons, the version."""
import importlib
import os
import re
import subprocess

from stabstitch2_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


def modules():
    """The binding modules, in the order of the package's list."""
    return [importlib.import_module('stabstitch2_amd.' + name) for name in _hip.LIBRARIES]


def built(module):
    """The loaded library of a binding module; everything is built first if its file is missing."""
    if not os.path.exists(module.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return module.lib()


def header(module):
    return open(os.path.join(ROOT, 'include', module.HEADER)).read()


def headers_before(module):
    """{header name: text} of the libraries in front of `module` in the package's list: the ones that must not know of it."""
    mods = modules()
    return {m.HEADER: header(m) for m in mods[:mods.index(module)]}


def declared(module):
    """The sorted names a header declares under its API macro."""
    return sorted(set(re.findall(r'\b%s[^;]*?\b(%s[a-z0-9_]+)\s*\(' % (module.API, module.PREFIX), header(module))))


def exported(path):
    """The sorted ' T ' symbols of `nm -D --defined-only` that do not start with '_'."""
    nm = subprocess.run(['nm', '-D', '--defined-only', path], check=True, capture_output=True, text=True).stdout
    return sorted(line.split()[-1] for line in nm.splitlines() if ' T ' in line and not line.split()[-1].startswith('_'))


def check(module):
    """Header declarations == ctypes table == exports; every declaration's parameter count == the length of its argtypes;
    <PREFIX>_ERR_ARG == the module's ERR_ARG == -1.  -> (declared names, the header's integer #defines)."""
    hdr = header(module)
    names = declared(module)
    assert names == sorted(module.SIGNATURES), sorted(set(names) ^ set(module.SIGNATURES))
    assert exported(module.LIB_PATH) == names, exported(module.LIB_PATH)                # nothing else leaves the library
    params = re.findall(r'\b%s[^;]*?\b(%s[a-z0-9_]+)\s*\(([^)]*)\)' % (module.API, module.PREFIX), hdr)
    assert sorted(name for name, _ in params) == names, params
    for name, text in params:
        count = 0 if text.strip() == 'void' else len(text.split(','))
        assert count == len(module.SIGNATURES[name][1]), name
    macro = module.PREFIX.upper()
    defines = {k: int(v) for k, v in re.findall(r'^#define (%s[A-Z_]+) (-?\d+)\b' % macro, hdr, re.M)}
    assert defines[macro + 'ERR_ARG'] == module.ERR_ARG == ERR_ARG
    return names, defines
