"""Code bytes and resources of the env-step kernels, per kernel, from built
code alone (no GPU):
  python scripts/kernel_code_size.py [libmas.so | device objects ...] [--all]
A shared library's gfx950 code objects are taken out of its offload bundles;
a device object is what `hipcc --cuda-device-only --no-gpu-bundle-output -c`
writes.  Code bytes are the kernels' symbol sizes (llvm-readelf -sW); VGPRs,
SGPRs, spills, scratch and LDS are the code object's own metadata note (what
-Rpass-analysis=kernel-resource-usage prints), and the waves per SIMD follow
from the VGPRs (512 per SIMD lane, allocated in blocks of 8, at most 8 waves).
Default: k_pre_lanes, k_gen_solve_g, k_post_lanes; --all: every kernel."""
import argparse
import os
import re
import struct
import subprocess
import sys
import tempfile

READELF = os.environ.get('LLVM_READELF', '/opt/rocm/llvm/bin/llvm-readelf')
MAGIC = b'__CLANG_OFFLOAD_BUNDLE__'


def code_objects(path):
    """(label, elf bytes) of a device object, or of every gfx950 entry of a library's bundles"""
    data = open(path, 'rb').read()
    if data[:4] == b'\x7fELF' and struct.unpack_from('<H', data, 18)[0] == 224:  # EM_AMDGPU
        return [(os.path.basename(path), data)]
    out = []
    at = data.find(MAGIC)
    while at >= 0:
        n = struct.unpack_from('<Q', data, at + len(MAGIC))[0]
        p = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from('<QQQ', data, p)
            triple = data[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if 'gfx950' in triple and size:
                out.append(('%s@%#x' % (os.path.basename(path), at + off), data[at + off:at + off + size]))
        at = data.find(MAGIC, p)
    if not out:
        sys.exit('%s: no gfx950 code object found (a compressed bundle is not handled)' % path)
    return out


def demangle(names):
    for tool in (os.path.join(os.path.dirname(READELF), 'llvm-cxxfilt'), 'c++filt'):
        try:
            r = subprocess.run([tool] + names, capture_output=True, text=True)
        except OSError:
            continue
        if r.returncode == 0:
            return r.stdout.splitlines()
    return names


def class_names(here):
    """'Cap<4, 4, 4, 4, 4>' -> '2v2', from the class units' `using CapClass_<name> = mas::Cap<...>;`"""
    out = {}
    src = os.path.join(here, '..', 'gym-ma-survival-2d_amd', 'csrc')
    for f in sorted(os.listdir(src)) if os.path.isdir(src) else []:
        if f.startswith('mas_k_') and f.endswith('.hip'):
            m = re.search(r'using CapClass_(\w+) = mas::(Cap<[^>]*>);', open(os.path.join(src, f)).read())
            if m:
                out[m.group(2)] = m.group(1)
    return out


def kernels_of(elf):
    with tempfile.NamedTemporaryFile(suffix='.elf') as f:
        f.write(elf)
        f.flush()
        syms = subprocess.run([READELF, '-sW', f.name], capture_output=True, text=True, check=True).stdout
        notes = subprocess.run([READELF, '--notes', f.name], capture_output=True, text=True, check=True).stdout
    size = {}
    for line in syms.splitlines():
        c = line.split()
        if len(c) >= 8 and c[3] == 'FUNC':
            size[c[7]] = int(c[2])
    out = []
    # the metadata note: one list item per kernel under amdhsa.kernels
    for item in re.split(r'\n  - (?=\.)', notes)[1:]:
        kv = dict(re.findall(r'^\s*(\.[a-z_]+):\s*(\S+)\s*$', item, flags=re.M))
        name = kv.get('.name', '').strip("'\"")
        if name not in size:
            continue
        out.append({'name': name, 'code': size[name], 'vgpr': int(kv.get('.vgpr_count', 0)),
                    'agpr': int(kv.get('.agpr_count', 0)), 'sgpr': int(kv.get('.sgpr_count', 0)),
                    'vspill': int(kv.get('.vgpr_spill_count', 0)), 'sspill': int(kv.get('.sgpr_spill_count', 0)),
                    'scratch': int(kv.get('.private_segment_fixed_size', 0)),
                    'lds': int(kv.get('.group_segment_fixed_size', 0))})
    return out


def main():
    ap = argparse.ArgumentParser()
    here = os.path.dirname(os.path.abspath(__file__))
    ap.add_argument('files', nargs='*',
                    default=[os.path.join(here, '..', 'gym-ma-survival-2d_amd', 'masurvival', '_lib', 'libmas.so')])
    ap.add_argument('--all', action='store_true')
    args = ap.parse_args()
    rows = []
    names = class_names(here)
    for path in args.files:
        for label, elf in code_objects(path):
            rows += kernels_of(elf)
    for r, d in zip(rows, demangle([r['name'] for r in rows])):
        r['pretty'] = re.sub(r'\(.*$', '', d.replace('void ', '').replace('mas::', '')).replace('> >', '>>')
        for cap, name in names.items():
            r['pretty'] = r['pretty'].replace(cap, name)
    if not args.all:
        rows = [r for r in rows if re.match(r'k_(pre_lanes|gen_solve_g|post_lanes)\b', r['pretty'])]
    rows.sort(key=lambda r: (re.sub(r'^\w+', '', r['pretty']), r['pretty']))
    print('%-28s %9s %5s %5s %7s %7s %8s %7s %5s' % ('kernel', 'code B', 'VGPRs', 'SGPRs', 'v-spill', 's-spill',
                                                    'scratch', 'LDS B', 'occ'))
    for r in rows:
        regs = max(r['vgpr'] + r['agpr'], 1)
        occ = min(8, 512 // (-(-regs // 8) * 8))
        print('%-28s %9d %5d %5d %7d %7d %8d %7d %5d' % (r['pretty'], r['code'], r['vgpr'], r['sgpr'], r['vspill'],
                                                        r['sspill'], r['scratch'], r['lds'], occ))


if __name__ == '__main__':
    main()
