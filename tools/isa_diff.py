#!/usr/bin/env python3
"""Which kernels did an edit touch?  Device-code comparison of two source trees, kernel by kernel, without a GPU.

    python tools/isa_diff.py OLD NEW [--files dmf_patch_v2.hip ...] [--changed] [--keep DIR] [--define D ...]

OLD and NEW are two checkouts of this repository (e.g. `git worktree add ../parent HEAD~1` and `.`).  For every file
(default: dmf_patch_v2.hip, dmf_reduce.hip, dmf_attention.hip) each tree's device-only assembly listing is made with
the flags that tree's build.py gives the file, and every kernel is reported as

    =|CHANGED   instructions   next_free_vgpr   next_free_sgpr   private_segment_fixed_size (scratch)   static LDS   name

with `old>new` where a figure moved.  Two kernels are identical when their listings agree line by line once comments,
blank lines and the numbering of local labels are stripped.  (Dynamic LDS is a launch argument and not in the listing.)
Exit status: 0 when both trees have the same set of kernels — changed or not —, 1 when the sets differ.
--keep DIR keeps the listings, named by a hash of the sources and flags, and reuses them on the next call.
"""
import argparse
import hashlib
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

FILES = ('dmf_patch_v2.hip', 'dmf_reduce.hip', 'dmf_attention.hip')
META = (('vgpr', '.amdhsa_next_free_vgpr'), ('sgpr', '.amdhsa_next_free_sgpr'),
        ('scratch', '.amdhsa_private_segment_fixed_size'), ('lds', '.amdhsa_group_segment_fixed_size'))
LOCAL_LABEL = re.compile(r'\.L(BB|func_end|func_begin|tmp|JTI)\d+')


def parse_listing(text):
    """{kernel: {'body': [normalised lines], 'insts': n, 'vgpr': .., 'sgpr': .., 'scratch': .., 'lds': ..}}"""
    lines = text.splitlines()
    kernels = {}
    for i, ln in enumerate(lines):
        t = ln.strip()
        if not t.startswith('.amdhsa_kernel '):
            continue
        name = t.split()[1]
        meta = {}
        for m in lines[i + 1:]:
            w = m.split()
            if w and w[0] == '.end_amdhsa_kernel':
                break
            for key, directive in META:
                if len(w) == 2 and w[0] == directive:
                    meta[key] = int(w[1], 0)
        kernels[name] = meta
    label = {ln.split(':')[0]: i for i, ln in enumerate(lines) if ln[:1] not in ('', '\t', ' ', '.', ';') and ':' in ln}
    for name, k in kernels.items():
        start = label[name]
        body, in_meta = [], False
        for ln in lines[start + 1:]:
            t = ln.split(';')[0].strip()
            if t.startswith('.Lfunc_end'):
                break
            if t.startswith('.amdhsa_kernel'):
                in_meta = True
            if not t or in_meta:
                in_meta = in_meta and not t.startswith('.end_amdhsa_kernel')
                continue
            body.append(LOCAL_LABEL.sub(lambda m: '.L' + m.group(1), t))
        k['body'] = body
        k['insts'] = sum(1 for t in body if not t.startswith('.') and not t.endswith(':'))
    return kernels


def compare(old, new):
    """rows (name, changed, {figure: (old, new)}) of the kernels both listings have, and the names only one has"""
    rows = []
    for name in old:
        if name in new:
            a, b = old[name], new[name]
            rows.append((name, a['body'] != b['body'], {f: (a.get(f), b.get(f)) for f in ('insts',) + tuple(k for k, _ in META)}))
    return rows, sorted(set(old) - set(new)), sorted(set(new) - set(old))


def demangle(names):
    tool = shutil.which('llvm-cxxfilt') or shutil.which('c++filt') or next(
        (p for p in ('/opt/rocm/llvm/bin/llvm-cxxfilt', '/opt/rocm/lib/llvm/bin/llvm-cxxfilt') if os.path.exists(p)), None)
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input='\n'.join(names) + '\n', capture_output=True, text=True).stdout.splitlines()
    if len(out) != len(names):
        return {n: n for n in names}
    # the return type and the parameter list say nothing the template arguments do not
    return {n: re.sub(r'^void ', '', d[:d.index('>(') + 1] if '>(' in d else d.split('(')[0]) for n, d in zip(names, out)}


def tree_build(tree):
    path = os.path.join(tree, 'dual-modal-fusion_amd', 'build.py')
    spec = importlib.util.spec_from_file_location('isa_diff_build_' + hashlib.sha1(path.encode()).hexdigest()[:8], path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def listing(tree, fname, keep, defines):
    """path of the device-only assembly listing of csrc/<fname> of `tree`, compiled with that tree's build.py flags"""
    b = tree_build(tree)
    src = os.path.join(b.HERE, 'csrc', fname)
    cmd = [os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')] + list(b.FLAGS) + list(b.EXTRA.get(fname, [])) + ['-D' + d for d in defines]
    h = hashlib.sha1(' '.join(cmd).encode())
    for p in [src] + list(b.HDR):
        h.update(open(p, 'rb').read())
    out = os.path.join(keep, '%s.%s.s' % (fname, h.hexdigest()[:12]))
    if not os.path.exists(out):
        print('# compiling %s of %s' % (fname, tree), file=sys.stderr, flush=True)
        r = subprocess.run(cmd + ['--cuda-device-only', '-S', src, '-o', out + '.tmp'], stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise SystemExit('%s of %s does not compile:\n%s' % (fname, tree, r.stderr))
        os.replace(out + '.tmp', out)
    return out


def fig(pair):
    return str(pair[0]) if pair[0] == pair[1] else '%s>%s' % pair


def report(fname, old, new, changed_only=False, out=sys.stdout):
    """prints the table of one file; True when both listings hold the same set of kernels"""
    rows, gone, added = compare(old, new)
    names = demangle([r[0] for r in rows] + gone + added)
    nch = sum(1 for r in rows if r[1])
    print('%s: %d kernels, %d identical, %d changed; instructions %d -> %d' % (
        fname, len(rows), len(rows) - nch, nch, sum(r[2]['insts'][0] for r in rows), sum(r[2]['insts'][1] for r in rows)), file=out)
    fmt = '  %-8s %-11s %-8s %-8s %-8s %-8s %s'
    print(fmt % ('', 'insts', 'vgpr', 'sgpr', 'scratch', 'lds', 'kernel'), file=out)
    for name, changed, figs in rows:
        if changed or not changed_only:
            figures = tuple(fig(figs[k]) for k in ('insts', 'vgpr', 'sgpr', 'scratch', 'lds'))
            print(fmt % (('CHANGED' if changed else '=',) + figures + (names[name],)), file=out)
    for n in gone:
        print('  ONLY IN OLD  %s' % names[n], file=out)
    for n in added:
        print('  ONLY IN NEW  %s' % names[n], file=out)
    return not gone and not added


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('old')
    ap.add_argument('new')
    ap.add_argument('--files', nargs='+', default=list(FILES))
    ap.add_argument('--changed', action='store_true', help='list only the kernels that changed')
    ap.add_argument('--keep', help='directory that keeps (and is searched for) the listings')
    ap.add_argument('--define', action='append', default=[], help='extra -D for both trees (e.g. DMF_STAMPS)')
    ap.add_argument('--jobs', type=int, default=min(6, os.cpu_count() or 1))
    args = ap.parse_args()
    keep = args.keep or tempfile.mkdtemp(prefix='isa_diff_')
    os.makedirs(keep, exist_ok=True)
    work = [(t, f) for f in args.files for t in (args.old, args.new)]
    try:
        with ThreadPoolExecutor(max_workers=max(1, args.jobs)) as ex:
            paths = dict(zip(work, ex.map(lambda w: listing(w[0], w[1], keep, args.define), work)))
        same = [report(f, *(parse_listing(open(paths[(t, f)]).read()) for t in (args.old, args.new)), changed_only=args.changed)
                for f in args.files]
        return 0 if all(same) else 1
    finally:
        if not args.keep:
            shutil.rmtree(keep, ignore_errors=True)


if __name__ == '__main__':
    sys.exit(main())
