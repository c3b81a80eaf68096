#!/usr/bin/env python3
"""Compare the gfx950 device code of every kernel against another git revision.  Needs hipcc, no GPU.

    python tools/isa_diff.py [REV] [--allow-missing NAME ...]

Every build.SOURCES entry of each revision is compiled to device assembly with build.py's flags; the assembly
is normalised (comments, .file/.ident, __hip_cuid_* lines, the zero-page symbol's name, per-file label numbers)
and split per function symbol.  Symbols are matched by name over all sources of a revision, so a kernel that moved
to another file compares against itself.  Prints the symbols that differ, are missing or are new, with the file(s)
they live in; exit status 1 when there is one outside --allow-missing (a substring of the mangled name is enough).
"""
import argparse
import ast
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from seg2eye_amd import build  # noqa: E402

DROP = re.compile(r'^\s*(\.file|\.ident)\b|__hip_cuid_')
SUBS = [(re.compile(r'\s*;.*$'), ''), (re.compile(r'\b_Z\w*zero16E?\b'), 'ZERO16'),
        (re.compile(r'\.L(BB|func_begin|func_end|tmp)\d+'), r'.L\1')]


def compile_asm(tree, src, out):
    path = os.path.join(tree, 'seg2eye_amd', 'csrc', src)
    if not os.path.exists(path):
        return None
    cmd = [build._hipcc(), '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC',
           '--offload-device-only', '-S', path, '-o', out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        sys.exit('hipcc failed on %s:\n%s' % (path, r.stdout.decode()))
    return out


def functions(asm_path):
    """{symbol: [normalised lines of its body and, for a kernel, its .amdhsa_kernel descriptor]}"""
    lines = []
    for ln in open(asm_path):
        if DROP.search(ln):
            continue
        for pat, rep in SUBS:
            ln = pat.sub(rep, ln)
        if ln.strip():
            lines.append(ln.rstrip())
    names = {m.group(1) for ln in lines for m in [re.match(r'\s*\.type\s+(\S+),@function', ln)] if m}
    out, cur = {}, None
    for ln in lines:
        s = ln.strip()
        if s.endswith(':') and s[:-1] in names:
            cur = out.setdefault(s[:-1], [])
        elif s.startswith('.amdhsa_kernel '):
            cur = out.setdefault(s.split()[1], [])
        if cur is not None:
            cur.append(ln)
        if s.startswith('.Lfunc_end') or s == '.end_amdhsa_kernel':
            cur = None
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('rev', nargs='?', default='HEAD~1')
    ap.add_argument('--allow-missing', nargs='*', default=[], metavar='NAME')
    ap.add_argument('--show', action='store_true', help='print a unified diff of each differing symbol')
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, 'old')
        os.makedirs(old)
        subprocess.check_call('git archive %s seg2eye_amd/csrc include | tar -x -C %s' % (args.rev, old),
                              shell=True, cwd=ROOT)
        # the sources of REV are its own build.SOURCES; a symbol is matched by name over all of them, whichever file holds it
        old_list = re.search(r'^SOURCES = (\[.*?\])', subprocess.check_output(
            ['git', 'show', args.rev + ':seg2eye_amd/build.py'], cwd=ROOT).decode(), re.M | re.S).group(1)
        jobs = [(tree, src, os.path.join(tmp, '%s_%s.s' % (tag, src)))
                for tag, tree, srcs in (('old', old, ast.literal_eval(old_list)), ('new', ROOT, build.SOURCES)) for src in srcs]
        with ThreadPoolExecutor(16) as ex:
            asm = list(ex.map(lambda j: compile_asm(*j), jobs))
        a, b = {}, {}                                        # {symbol: (file, body)} at REV and now
        for (tree, src, _), p in zip(jobs, asm):
            (a if tree == old else b).update({name: (src, body) for name, body in (functions(p) if p else {}).items()})
        bad = 0
        for name in sorted(set(a) | set(b), key=lambda n: ((a.get(n) or b[n])[0], n)):
            what = 'missing' if name not in b else 'new' if name not in a else 'differs' if a[name][1] != b[name][1] else None
            if what is None:
                continue
            allowed = what == 'missing' and any(x in name for x in args.allow_missing)
            bad += not allowed
            where = ' -> '.join(dict.fromkeys(m[name][0] for m in (a, b) if name in m))
            print('%-8s %s: %s%s' % (what, where, name, '  (allowed)' if allowed else ''))
            if what == 'differs' and args.show:
                print('\n'.join(difflib.unified_diff(a[name][1], b[name][1], 'old', 'new', lineterm='', n=2)))
        moved = sum(a[n][0] != b[n][0] for n in set(a) & set(b))
        print('%d symbols at %s, %d now, %d in another file' % (len(a), args.rev, len(b), moved), file=sys.stderr)
    print('isa_diff vs %s: %s' % (args.rev, 'identical' if not bad else '%d difference(s)' % bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
