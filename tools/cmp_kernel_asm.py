"""Compare the device assembly of one translation unit at two commits kernel by kernel, for a refactor that must not change
device code but may change the order in which template instantiations come out.

  hipcc <the unit's flags> --cuda-device-only -S unit.hip -o a.s     (at each commit)
  python tools/cmp_kernel_asm.py parent.s new.s

The text sections are keyed by symbol, the metadata entries by kernel name; what depends on a function's position in the file (the
function number in block labels and the padding it leaves in front of a label's comment, .Lfunc_begin / .Lfunc_end) and the
compilation unit id are normalised away.  Exit status 0: the same symbols, every body and every metadata entry identical; a
change that adds kernels exits 1 and lists them, and nothing else may be listed."""
import re
import sys


def load(path):
    txt = open(path).read()
    cut = txt.index('\t.amdgpu_metadata')
    parts = re.split(r'(?m)^(?=\t\.section\t\.text\.)', txt[:cut])
    bodies = {}
    for c in parts[1:]:
        name = re.match(r'\t\.section\t\.text\.([^,]+),', c).group(1)
        c = re.sub(r'\bBB\d+_', 'BB_', re.sub(r'\.LBB\d+_', '.LBB_', c))
        c = re.sub(r'\.Lfunc_(begin|end)\d+', r'.Lfunc_\1', c)
        c = re.sub(r'(?m)^(\.LBB_\d+:)[ \t]+;', r'\1 ;', c)      # a label's comment is padded to a column: a function number one digit longer moves it
        bodies[name] = bodies.get(name, '') + re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid', c)
    meta = re.split(r'(?m)^(?=  - \.)', txt[cut:])
    entries = {}
    for m in meta[1:]:
        n = re.search(r'\.name:\s+(\S+)', m)
        entries[n.group(1) if n else m[:60]] = m.strip()
    return parts[0], bodies, meta[0], entries


def main():
    ha, ba, ma, ea = load(sys.argv[1])
    hb, bb, mb, eb = load(sys.argv[2])
    bad = sorted(n for n in set(ba) | set(bb) if ba.get(n) != bb.get(n))
    badm = sorted(n for n in set(ea) | set(eb) if ea.get(n) != eb.get(n))
    print('%d / %d text sections, %d / %d metadata entries' % (len(ba), len(bb), len(ea), len(eb)))
    print('differing bodies: %d %s' % (len(bad), bad[:5]))
    print('of them in both files: %s; only in the first: %d, only in the second: %d' % (
        sorted(n for n in bad if n in ba and n in bb), sum(n not in bb for n in bad), sum(n not in ba for n in bad)))
    print('differing metadata entries: %d %s' % (len(badm), badm[:5]))
    print('file head identical: %s, metadata head identical: %s' % (ha == hb, ma == mb))
    sys.exit(0 if not bad and not badm and ha == hb and ma == mb else 1)


if __name__ == '__main__':
    main()
