#!/bin/bash
# Device code of one .hip file in two source trees, kernel by kernel: compiles both to gfx950 assembly with the flags
# _build.py gives that file (FLAGS and its EXTRA_FLAGS entry, read from each tree's own _build.py: the code that ships),
# drops comments / directives / metadata, renumbers the local labels and says per kernel whether the instruction streams are identical.  What a host-side refactor has to show (the kernels did not move) --
# a differing kernel is listed with the index of its first differing instruction and of its last v_mfma: a difference
# behind the last v_mfma left the K loop alone.  The offset of an LDS read is compared as a number: an explicit `offset:0`
# counts as none and `offset:0x800` as `offset:2048` (inline assembly prints what its author or the compiler spelled).
#     bash tools/device_code_diff.sh gemm_ring.hip /path/to/parent/tree [/path/to/this/tree] [-v]
# -v prints a unified diff of every differing kernel.  Kernels present in one tree only are listed as such; the
# instantiations of a template that gained ONE parameter (and, with it, trailing kernel arguments) are paired with the
# old kernel of the remaining parameters: the nearest of them is compared with it, the others are listed as new.
f=$1; old=$2; new=${3:-$(dirname "$(dirname "$(realpath "$0")")")}; verbose=0
for a in "$@"; do [ "$a" = "-v" ] && verbose=1; done
[ "$new" = "-v" ] && new=$(dirname "$(dirname "$(realpath "$0")")")
tmp=$(mktemp -d); trap 'rm -rf "$tmp"' EXIT
for side in old new; do
  root=${!side}
  # the flags each tree builds the file with: its own _build.FLAGS + _build.EXTRA_FLAGS[file] (the one list there is)
  flags=$(python3 -c 'import sys; sys.path.insert(0, sys.argv[1]); import _build; print(" ".join(_build.FLAGS + _build.EXTRA_FLAGS.get(sys.argv[2], [])))' \
    "$root/w2v2_speaker_amd" "$f") || exit 1
  /opt/rocm/bin/hipcc $flags --cuda-device-only -S \
    "$root/w2v2_speaker_amd/csrc/$f" -o "$tmp/$side.s" 2>"$tmp/$side.err" || { cat "$tmp/$side.err"; exit 1; }
done
python3 - "$tmp/old.s" "$tmp/new.s" "$verbose" "$f" <<'P'
import difflib, re, sys

def kernels(path):
    out, cur, body = {}, None, []
    for l in open(path):
        l = l.rstrip()
        m = re.match(r'^(_Z\w+):', l)
        if m and cur is None:
            cur, body = m.group(1), []
            continue
        if cur is None:
            continue
        s = l.split(';')[0].strip()               # comments carry line numbers and register statistics
        if not s or s.startswith('.') and not s.startswith(('.LBB', '.Lpost_getpc')):
            continue
        if s.startswith('ds_read'):                  # one encoding, three spellings: none / offset:0, offset:2048 / offset:0x800
            s = re.sub(r'\s+offset:(0x[0-9a-f]+|\d+)$', lambda m: ' offset:%d' % int(m.group(1), 0) if int(m.group(1), 0) else '', s)
        body.append(s)
        if s == 's_endpgm':
            # local labels are numbered per translation unit: renumber in order of appearance
            names = {}
            def ren(m):
                return names.setdefault(m.group(0), 'L%d' % len(names))
            out[cur] = [re.sub(r'\.LBB\d+_\d+|\.Lpost_getpc\d+', ren, x) for x in body]
            cur = None
    return out

old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
verbose = sys.argv[3] == '1'
# a kernel template that GAINED one parameter: its instantiations are compared with the old kernel of the remaining ones
# (listed under the new name)
for n in [k for k in new if k not in old]:
    for m in reversed(list(re.finditer(r'L[bi]\d+E', n))):      # a trailing parameter first
        o = (n[:m.start()] + n[m.end():]).replace('IEv', '', 1)    # (its only parameter: the old kernel was no template)
        # the new parameter may bring kernel arguments with it, appended to the old list: the old name is a prefix then
        c = max((k for k in old if k not in new and o.startswith(k)), key=len, default=None)
        if c is not None and o not in new:
            old[n] = old[c]
            break
for o in [k for k in old if k not in new and any(old[k] is old.get(n) for n in new)]:
    # several instantiations of the new template: the old kernel is compared with the nearest, the others are new code
    pairs = [n for n in new if old.get(n) is old[o]]
    near = max(pairs, key=lambda n: difflib.SequenceMatcher(None, old[o], new[n], autojunk=False).ratio())
    for n in pairs:
        if n != near: del old[n]
    del old[o]
same = [k for k in old if k in new and old[k] == new[k]]
diff = [k for k in old if k in new and old[k] != new[k]]
print(f"{sys.argv[4]}: {len(old)} kernels before, {len(new)} after; {len(same)} identical, {len(diff)} differing, "
      f"{len([k for k in old if k not in new])} only before, {len([k for k in new if k not in old])} only after")
for k in diff:
    d = list(difflib.unified_diff(old[k], new[k], lineterm='', n=2))
    plus = sum(1 for x in d if x.startswith('+') and not x.startswith('+++'))
    minus = sum(1 for x in d if x.startswith('-') and not x.startswith('---'))
    first = next((i for i, (x, y) in enumerate(zip(old[k], new[k])) if x != y), min(len(old[k]), len(new[k])))
    last_mfma = [max((i for i, x in enumerate(v) if x.startswith('v_mfma')), default=-1) for v in (old[k], new[k])]
    print(f"  DIFFERS {k}: {len(old[k])} -> {len(new[k])} instructions (-{minus} +{plus}); first difference at "
          f"instruction {first}, last v_mfma at {last_mfma[0]} -> {last_mfma[1]}")
    if verbose:
        print('\n'.join('      ' + x for x in d))
for k in old:
    if k not in new: print(f"  ONLY BEFORE {k}: {len(old[k])} instructions")
for k in new:
    if k not in old: print(f"  ONLY AFTER  {k}: {len(new[k])} instructions")
P
