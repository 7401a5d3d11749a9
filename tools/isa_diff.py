#!/usr/bin/env python3
"""Compare two `make -C trace-of-radiance_amd/csrc asm` outputs kernel by kernel (round 5: pruning the variant table must not
change a kept variant).  Labels carry the function's ordinal in the file (.LBB57_12), which shifts when functions are removed:
they are normalised; everything else must match byte for byte.  The resource fields of each kernel's `amdhsa.kernels` metadata
entry (registers, scratch, LDS, kernarg size, workgroup size) must match too.

    python tools/isa_diff.py old.s new.s [--rename OLD=NEW ...]

--rename OLD=NEW (repeatable): a kernel of old.s whose mangled name contains OLD is compared, as a kept kernel, with the kernel of
new.s of that name with OLD replaced by NEW; each kernel's own name is normalised inside its body.  Text comparison only.
"""
import argparse
import re
import sys

META = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size", ".kernarg_segment_size",
        ".max_flat_workgroup_size")
FUNCS = set()


def kernels(path):
    """{mangled name: body lines}, the kernel's own name replaced by <self>; the names typed @function go into FUNCS (every
    other symbol, such as a constant table, is compared as text alone and has no metadata entry)"""
    out, name, body = {}, None, []
    for ln in open(path):
        f = re.match(r"^\s*\.type\s+(_Z\w+),@function", ln)
        if f:
            FUNCS.add(f.group(1))
        m = re.match(r"^(_Z\w+):\s", ln)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if ln.startswith("\t.section") or ln.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        t = re.sub(r"\.LBB\d+_", ".LBB_", ln)
        t = re.sub(r";.*$", "", t).rstrip()      # comments carry block ordinals too
        t = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", t)
        t = t.replace(name, "<self>")
        if t:
            body.append(t)
    return out


def metadata(path):
    """{mangled name: {field: value}} for the META fields of the entries of the amdhsa.kernels list"""
    out, cur, inside = {}, None, False
    for ln in open(path):
        if ln.startswith("amdhsa.kernels:"):
            inside = True
            continue
        if not inside:
            continue
        if not ln.startswith("  "):  # the next top-level key, or the end of the document
            inside = False
            continue
        m = re.match(r"^(  - |    )(\.\w+):\s+(\S+)\s*$", ln)  # an entry's own fields: nested lists sit deeper
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        if m.group(2) == ".name":
            out[m.group(3)] = cur
        elif m.group(2) in META:
            cur[m.group(2)] = m.group(3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    args = ap.parse_args()
    a, b = kernels(args.old), kernels(args.new)
    ma, mb = metadata(args.old), metadata(args.new)
    pair = {}  # old name -> new name
    for k in a:
        to = k
        for r in args.rename:
            old, new = r.split("=", 1)
            if old in k and k.replace(old, new) in b and k not in b:
                to = k.replace(old, new)
                break
        if to in b:
            pair[k] = to
    renamed = sorted(k for k in pair if pair[k] != k)
    gone = sorted(set(a) - set(pair))
    new = sorted(set(b) - set(pair.values()))
    diff = []
    for k in sorted(pair):
        body = a[k] != b[pair[k]]
        # a kernel without a parsed field on either side differs: an unreadable metadata block must not pass as equal
        x, y = ma.get(k, {}), mb.get(pair[k], {})
        meta = [f for f in META if x.get(f) != y.get(f) or x.get(f) is None] if k in FUNCS else []
        if body or meta:
            diff.append((k, body, meta))
    print(f"{len(a)} kernels before, {len(b)} after; removed {len(gone)}, added {len(new)}, kept {len(pair)} "
          f"({len(renamed)} renamed), kept-but-different {len(diff)}")
    for k in gone:
        print("  removed:", k)
    for k in new:
        print("  added:  ", k)
    for k in renamed:
        print("  renamed:", k, "->", pair[k])
    for k, body, meta in diff:
        x, y = a[k], b[pair[k]]
        n = sum(1 for p, q in zip(x, y) if p != q) + abs(len(x) - len(y))
        print(f"  DIFFERS: {k}: {len(x)} -> {len(y)} lines, {n} differing" +
              "".join(f"; {f} {ma.get(k, {}).get(f)} -> {mb.get(pair[k], {}).get(f)}" for f in meta))
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
