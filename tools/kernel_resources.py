"""Registers, spills, scratch and argument-block bytes of every kernel of a build, read from the code objects' metadata -- no GPU needed.
What the static_asserts on the kernels' argument blocks point to: growing a block, or adding a value that lives across a kernel, is checked
here against the build it came from before anything is timed.
usage: python tools/kernel_resources.py [OBJDIR]                 one line per kernel of the objects in OBJDIR (default: the newest object per
                                                                 source in build/objcache of this checkout)
       python tools/kernel_resources.py OBJDIR --against OTHER   only the kernels whose vector / accumulator registers, spills or scratch
                                                                 differ from OTHER's (another checkout's build/objcache), and how many
                                                                 scalar register counts moved
Needs the LLVM tools that ship with ROCm (llvm-objcopy, clang-offload-bundler, llvm-readelf; $ROCM_PATH/llvm/bin, default /opt/rocm)."""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin')
FIELDS = (('v', 'vgpr_count'), ('a', 'agpr_count'), ('s', 'sgpr_count'), ('vspill', 'vgpr_spill_count'), ('sspill', 'sgpr_spill_count'),
          ('scratch', 'private_segment_fixed_size'), ('kernarg', 'kernarg_segment_size'), ('lds', 'group_segment_fixed_size'))
SHOWN = ('v', 'a', 'vspill', 'sspill', 'scratch')


def newest_objects(objdir):
    """{source name: path} -- the newest object of each source (the cache keeps one per content hash)."""
    best = {}
    for p in glob.glob(os.path.join(objdir, '*.o')):
        src = os.path.basename(p).split('.')[0]
        if src not in best or os.path.getmtime(p) > os.path.getmtime(best[src]):
            best[src] = p
    return best


def kernels_of(obj, arch='gfx950'):
    """{kernel symbol: {field: int}} of one host object with an embedded device bundle."""
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, 'fat.bin'), os.path.join(tmp, 'dev.co')
        subprocess.run([os.path.join(LLVM, 'llvm-objcopy'), f'--dump-section=.hip_fatbin={fat}', obj, os.path.join(tmp, 'copy.o')], check=True, capture_output=True)
        subprocess.run([os.path.join(LLVM, 'clang-offload-bundler'), '--type=o', f'--targets=hipv4-amdgcn-amd-amdhsa--{arch}', f'--input={fat}', f'--output={co}',
                        '--unbundle'], check=True, capture_output=True)
        notes = subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '--notes', co], check=True, capture_output=True, text=True).stdout
    out = {}
    for blk in re.split(r'\n\s+- \.agpr_count:', '\n' + notes)[1:]:
        blk = '.agpr_count:' + blk
        name = re.search(r'\.name:\s*(\S+)', blk)
        if name:
            out[name.group(1)] = {k: int((re.search(r'\.' + f + r':\s*(\d+)', blk) or [0, -1])[1]) for k, f in FIELDS}
    return out


def build_table(objdir):
    table = {}
    for src, obj in sorted(newest_objects(objdir).items()):
        for k, v in kernels_of(obj).items():
            table[(src, k)] = v
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('objdir', nargs='?', default=os.path.join(ROOT, 'build', 'objcache'))
    ap.add_argument('--against', default=None)
    args = ap.parse_args()
    mine = build_table(args.objdir)
    if not mine:
        sys.exit(f'no objects under {args.objdir}: build first (python -m codeformer_amd.build)')
    if args.against is None:
        for (src, k), v in sorted(mine.items()):
            print(src, k, ' '.join(f'{f} {v[f]}' for f, _ in FIELDS))
        return
    other = build_table(args.against)
    print(f'{len(mine)} kernels here, {len(other)} there; only here: {sorted(set(mine) - set(other))}; only there: {sorted(set(other) - set(mine))}')
    moved, blocks = 0, {}
    for key in sorted(set(mine) & set(other)):
        a, b = other[key], mine[key]
        ch = {f: (a[f], b[f]) for f in SHOWN if a[f] != b[f]}
        moved += a['s'] != b['s']
        if a['kernarg'] != b['kernarg']:
            blocks.setdefault((key[0], a['kernarg'], b['kernarg']), []).append(key[1])
        if ch:
            print(key[0], key[1], ' '.join(f'{f} {x} -> {y}' for f, (x, y) in ch.items()))
    for (src, x, y), ks in sorted(blocks.items()):
        print(f'{src}: argument segment {x} -> {y} bytes in {len(ks)} kernels')
    print(f'scalar register count differs in {moved} of {len(set(mine) & set(other))} kernels')


if __name__ == '__main__':
    main()
