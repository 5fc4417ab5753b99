"""Is the gfx950 device code of two builds of the kernel library the same, instruction for instruction?

    python tools/isa_diff.py [--rename REGEX=REPL]... LIB_A LIB_B

Unbundles both libraries (llvm-objdump --offloading), disassembles every gfx950 code object (llvm-objdump -d) and compares the two
listings as plain text.  Prints an md5 per side and the symbols whose listings differ (with the number of differing lines); exit
status 1 on any difference.  The acceptance check of a refactor: identical device code is unchanged speed by construction.
--rename (re.sub on the symbol names of LIB_A, before the comparison) is for a refactor that changes a kernel's template parameters and
with them its mangled name: the whole listings then differ, and the verdict is `identical per symbol`."""
import difflib
import glob
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile


def _objdump():
    for cand in (os.environ.get('LLVM_OBJDUMP'), '/opt/rocm/llvm/bin/llvm-objdump', shutil.which('llvm-objdump')):
        if cand and os.path.exists(cand):
            return cand
    raise SystemExit('llvm-objdump not found (set LLVM_OBJDUMP)')


def listing(lib):
    """{symbol: [instruction lines]} over all gfx950 code objects of `lib`, and the whole text."""
    od = _objdump()
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(lib, os.path.join(tmp, 'lib.so'))
        subprocess.run([od, '--offloading', 'lib.so'], cwd=tmp, check=True, stdout=subprocess.DEVNULL)
        objs = sorted(glob.glob(os.path.join(tmp, 'lib.so.*gfx950')), key=lambda p: int(os.path.basename(p).split('.')[2]))
        if not objs:
            raise SystemExit(f'{lib}: no gfx950 code object')
        text = []
        for k, o in enumerate(objs):
            out = subprocess.run([od, '-d', os.path.basename(o)], cwd=tmp, check=True, capture_output=True, text=True).stdout
            text.append(f'== code object {k}\n' + '\n'.join(ln for ln in out.splitlines() if 'file format' not in ln))
    text = '\n'.join(text)
    syms, cur = {}, None
    for ln in text.splitlines():
        m = re.match(r'^[0-9a-f]+ <(.+)>:$', ln)
        if m:
            cur = syms.setdefault(m.group(1), [])
        elif ln.startswith(('== code object', 'Disassembly of section')):
            cur = None      # the last symbol of a code object ends here, not at the next object's first symbol
        elif cur is not None and ln.strip() and ln.strip() != '...':      # ('...': zero padding behind a code object's last symbol)
            cur.append(ln.split('//')[0].rstrip())      # per symbol: the instructions without their addresses (code that only moved is the same)
    return syms, text


def main():
    args, renames = sys.argv[1:], []
    while len(args) > 1 and args[0] == '--rename':
        renames.append(args[1].split('=', 1))
        args = args[2:]
    if len(args) != 2 or any(len(r) != 2 for r in renames):
        raise SystemExit(__doc__)
    (sa, ta), (sb, tb) = listing(args[0]), listing(args[1])
    for lib, t in ((args[0], ta), (args[1], tb)):
        print(f'{hashlib.md5(t.encode()).hexdigest()}  {lib}  ({len(t.splitlines())} lines)')
    if ta == tb:
        print('identical')
        return 0
    for pat, repl in renames:
        renamed = {re.sub(pat, repl, name): ins for name, ins in sa.items()}
        if len(renamed) != len(sa):
            raise SystemExit(f'--rename {pat}={repl} maps two symbols of LIB_A to one name')
        sa = renamed
    bad = 0
    for name in sorted(set(sa) | set(sb)):
        a, b = sa.get(name), sb.get(name)
        if a is None or b is None:
            print(f'only in {"B" if a is None else "A"}: {name}')
        elif a != b:
            n = sum(1 for d in difflib.unified_diff(a, b, n=0, lineterm='') if d[0] in '+-' and d[:3] not in ('+++', '---'))
            print(f'differs ({len(a)} / {len(b)} instructions, {n} lines of diff): {name}')
        bad += a != b
    if renames and not bad:
        print(f'identical per symbol ({len(sb)} symbols, after the renames)')
        return 0
    print('DIFFERENT')
    return 1


if __name__ == '__main__':
    sys.exit(main())
