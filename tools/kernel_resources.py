#!/usr/bin/env python
"""Register / scratch / LDS budget of every gfx950 kernel in a built library, read from the code objects' metadata notes:
    python tools/kernel_resources.py [stabstitch2_amd/libstabstitch_hip.so] [name-substring]
The .so carries one clang offload bundle per translation unit in its .hip_fatbin section; each bundle's gfx950 entry is an ELF
whose NT_AMDGPU_METADATA note lists, per kernel, .vgpr_count / .agpr_count / .sgpr_count / .vgpr_spill_count / .sgpr_spill_count /
.private_segment_fixed_size (scratch bytes per lane) / .group_segment_fixed_size (static LDS).  tests/test_host_logic.py holds the
MFMA kernels to zero spills and zero scratch with `kernels()` below.

    python tools/kernel_resources.py --digest [lib]            per kernel: sha256 of its instruction stream, demangled name
    python tools/kernel_resources.py --digest-masked [lib]     the same with the offsets of the kernel-argument loads masked
The check for a source-only edit of the kernels (dead code removed, a template parameter renamed): build the library before and
after with the same compiler and compare the lists -- equal digests are equal machine code.  An edit that moves fields of a
kernel's argument struct shifts the offsets of its argument loads and nothing else: compare the masked lists (and the register /
LDS budgets of the table above)."""
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = '/opt/rocm/lib/llvm/bin'
MAGIC = b'__CLANG_OFFLOAD_BUNDLE__'


def code_objects(lib_path):
    """-> list of bytes: the gfx950 ELF of every bundle in the library's .hip_fatbin section."""
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, 'fatbin')
        subprocess.run([os.path.join(LLVM, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fat, lib_path, os.path.join(d, 'x')],
                       check=True, capture_output=True)
        blob = open(fat, 'rb').read()
    out = []
    pos = blob.find(MAGIC)
    while pos >= 0:
        n, = struct.unpack_from('<Q', blob, pos + len(MAGIC))
        q = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from('<QQQ', blob, q)
            triple = blob[q + 24:q + 24 + tlen].decode()
            q += 24 + tlen
            if 'gfx950' in triple and size:
                out.append(blob[pos + off:pos + off + size])
        pos = blob.find(MAGIC, pos + len(MAGIC))
    return out


_FIELDS = ('.vgpr_count', '.agpr_count', '.sgpr_count', '.vgpr_spill_count', '.sgpr_spill_count', '.private_segment_fixed_size',
           '.group_segment_fixed_size', '.max_flat_workgroup_size')


def kernels(lib_path):
    """-> {kernel name (demangled where llvm-cxxfilt knows it): {field: int}} over every gfx950 code object of the library,
    plus 'uses_mfma': whether the kernel's disassembly contains a v_mfma instruction."""
    res = {}
    with tempfile.TemporaryDirectory() as d:
        for i, elf in enumerate(code_objects(lib_path)):
            f = os.path.join(d, 'co%d.elf' % i)
            open(f, 'wb').write(elf)
            notes = subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '--notes', f], check=True, capture_output=True, text=True).stdout
            cur = None
            entries = []
            for line in notes.splitlines():
                m = re.match(r'^  - (\.[a-z_]+):\s*(.*)$', line)          # first key of a kernel entry
                if m:
                    cur = {}
                    entries.append(cur)
                else:
                    m = re.match(r'^    (\.[a-z_]+):\s*(.*)$', line)      # kernel-level key (argument entries sit deeper)
                if not m or cur is None:
                    continue
                k, v = m.group(1), m.group(2).strip()
                if k in _FIELDS:
                    cur[k] = int(v)
                elif k in ('.name', '.symbol'):
                    cur[k] = v.strip("'\"")
            # which kernels contain matrix instructions
            dis = subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '-d', f], check=True, capture_output=True, text=True).stdout
            mfma = {}
            sym = None
            for line in dis.splitlines():
                m = re.match(r'^[0-9a-f]+ <([^>]+)>:', line)
                if m:
                    sym = m.group(1)
                    mfma.setdefault(sym, 0)
                elif sym is not None and 'v_mfma' in line:
                    mfma[sym] += 1
            for e in entries:
                sym = e.get('.symbol', '')
                base = sym[:-3] if sym.endswith('.kd') else sym
                name = e.get('.name', base)
                e['mfma_instructions'] = mfma.get(base, 0)
                res[name] = e
    return _demangled(res)


def _demangled(by_symbol):
    names = list(by_symbol)
    for tool in (os.path.join(LLVM, 'llvm-cxxfilt'), 'c++filt'):      # (not every ROCm install carries llvm-cxxfilt)
        try:
            dem = subprocess.run([tool] + names, check=True, capture_output=True, text=True).stdout.splitlines()
            if len(dem) == len(names):
                return {d_: by_symbol[n] for d_, n in zip(dem, names)}
        except Exception:
            pass
    return by_symbol


def digests(lib_path, mask_kernarg_offsets=False):
    """-> {demangled kernel name: sha256 hex digest of its instruction stream}: mnemonics and operands in order, without addresses,
    encodings, comments and the fill behind its last instruction (branch operands are relative, so a kernel's digest does not depend
    on where it lies, nor on whether it is a template: those get sections of their own, zero-filled instead of s_nop-filled).
    mask_kernarg_offsets: the immediate offset of every scalar load whose base is the kernel-argument pointer (the user SGPR pair
    the kernel descriptor assigns to it) reads `KARG`."""
    res, pad = {}, {}
    with tempfile.TemporaryDirectory() as d:
        for i, elf in enumerate(code_objects(lib_path)):
            f = os.path.join(d, 'co%d.elf' % i)
            open(f, 'wb').write(elf)
            # kernel descriptors: which kernels there are, and the SGPR pair that holds the kernel-argument pointer at entry
            # (user SGPRs in the order private segment buffer (4), dispatch pointer (2), queue pointer (2), kernel arguments (2))
            kd = subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '-D', '-j', '.rodata', f], check=True, capture_output=True, text=True).stdout
            karg = {}
            sym = None
            for line in kd.splitlines():
                m = re.match(r'^\.amdhsa_kernel (\S+)', line)
                if m:
                    sym = m.group(1)
                    karg[sym] = 0
                    continue
                m = re.match(r'^\s*\.amdhsa_user_sgpr_(private_segment_buffer|dispatch_ptr|queue_ptr) (\d+)', line)
                if m and sym is not None and int(m.group(2)):
                    karg[sym] += 4 if m.group(1) == 'private_segment_buffer' else 2
            dis = subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '-d', '--no-show-raw-insn', f], check=True, capture_output=True, text=True).stdout
            sym = None
            for line in dis.splitlines():
                m = re.match(r'^[0-9a-f]+ <([^>]+)>:', line)
                if m:
                    sym = m.group(1) if m.group(1) in karg else None
                    if sym is not None:
                        res[sym] = hashlib.sha256()
                        base = 's[%d:%d]' % (karg[sym], karg[sym] + 1)
                        pad[sym] = []
                    continue
                ins = ' '.join(line.split('//')[0].split())
                if sym is None or not ins:
                    continue
                # the fill between a kernel's last instruction and the next symbol (s_nop rows from the assembler, or zeros that
                # objdump prints as `...`, whichever the kernel's section got) says where the kernel lies, not what it does: held
                # back, and hashed only if an instruction follows
                if ins in ('s_nop 0', '...'):
                    pad[sym].append(ins)
                    continue
                for held in pad[sym]:
                    res[sym].update((held + '\n').encode())
                pad[sym] = []
                if mask_kernarg_offsets:
                    m = re.match(r'^(s_load_dword\w* \S+ ' + re.escape(base) + r',) \S+(.*)$', ins)
                    if m:
                        ins = m.group(1) + ' KARG' + m.group(2)
                res[sym].update((ins + '\n').encode())
    return _demangled({k: v.hexdigest() for k, v in res.items()})


def main():
    args = sys.argv[1:]
    default_lib = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'stabstitch2_amd', 'libstabstitch_hip.so')
    if args and args[0] in ('--digest', '--digest-masked'):
        ds = digests(args[1] if len(args) > 1 else default_lib, mask_kernarg_offsets=args[0] == '--digest-masked')
        for name in sorted(ds):
            print('%s  %s' % (ds[name], name))
        return
    lib = args[0] if args and not args[0].startswith('-') else default_lib
    pat = args[1] if len(args) > 1 else ''
    ks = kernels(lib)
    print('%-100s %5s %5s %5s %6s %8s %7s %5s' % ('kernel', 'vgpr', 'agpr', 'sgpr', 'spill', 'scratch', 'lds', 'mfma'))
    for name in sorted(ks):
        if pat and pat not in name:
            continue
        e = ks[name]
        print('%-100s %5d %5d %5d %6d %8d %7d %5d' % (name[:100], e.get('.vgpr_count', -1), e.get('.agpr_count', 0), e.get('.sgpr_count', -1),
                                                     e.get('.vgpr_spill_count', 0) + e.get('.sgpr_spill_count', 0),
                                                     e.get('.private_segment_fixed_size', 0), e.get('.group_segment_fixed_size', 0),
                                                     e['mfma_instructions']))


if __name__ == '__main__':
    main()
