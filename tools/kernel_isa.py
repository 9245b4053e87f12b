#!/usr/bin/env python3
"""Disassembly of the built HIP objects' gfx950 code.
  python tools/kernel_isa.py <object stem, e.g. kernels> <mangled-name substring>     print the functions whose name matches
  python tools/kernel_isa.py --compare <other build dir> [--diff] [--rename OLD=NEW]... [--rename-file FILE]
                                                                                       is every function's instruction stream the same?
--compare: every kernel and every non-inlined device function of build/*.hip.o against those of another tree's build directory, by
mangled name across ALL objects (so code may move between translation units; a helper that is not inlined may sit in several
objects, and every copy has to equal the other tree's).  Two things are normalised, both link layout and not code: the s_nop
padding after a function's last instruction, and the 32-bit literals of the s_add_u32 / s_addc_u32 pair after an s_getpc_b64 (the
distance to a callee or a constant).  A function whose mangled name changed for a reason that is not code (a parameter's type moved to
another namespace) is paired by hand: --rename OLD=NEW, OLD being the other tree's name (or --rename-file: such a pair a line); it is
then compared like the rest and listed as renamed.  Names are never paired by guessing: one that is missing on either side without a
rename fails.  Exit code 1 if a name is missing on either side or a function differs; --diff prints how."""
import difflib, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
BUILD = os.path.join(ROOT, "hp-adaptive-signed-distance-field-octree_amd", "build")


def disassemble(obj):
    """{mangled name: [instruction lines]} of the object's gfx950 code object"""
    with tempfile.TemporaryDirectory() as td:
        fat, co = os.path.join(td, "fat.bin"), os.path.join(td, "k.co")
        # (an output file is named: with the input alone llvm-objcopy rewrites it in place, and the fresh time stamp hides later header edits from build.py)
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, os.path.join(td, "copy.o")], check=True, capture_output=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True, capture_output=True)
        dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], capture_output=True, text=True).stdout
    out = {}
    for blk in re.split(r"\n(?=[0-9a-f]+ <)", dis):
        head, _, body = blk.partition("\n")
        m = re.match(r"[0-9a-f]+ <(.+)>:$", head)
        if m and not m.group(1).endswith(".kd"):
            out[m.group(1)] = body.rstrip("\n").split("\n")
    return out


def normalised(lines):
    """the instructions without their addresses and encodings (branch targets stay, as <function+offset>), minus the two layout matters"""
    ins = []
    for ln in lines:
        text, _, comment = ln.partition("//")
        text = text.strip()
        if not text or text == "...":
            continue
        target = re.search(r"<[^>]+>\s*$", comment)
        ins.append(text + (" " + target.group(0).strip() if target else ""))
    while ins and ins[-1].startswith("s_nop"):
        ins.pop()
    for i, t in enumerate(ins):
        if t.startswith("s_getpc_b64") and i + 2 < len(ins) and ins[i + 1].startswith("s_add_u32") and ins[i + 2].startswith("s_addc_u32"):
            ins[i + 1] = ins[i + 1].rsplit(",", 1)[0] + ", <pc-relative>"
            ins[i + 2] = ins[i + 2].rsplit(",", 1)[0] + ", <pc-relative>"
    return ins


def functions(objdir):
    """{name: [(object, normalised instructions)]} over every *.hip.o of a build directory"""
    out = {}
    for f in sorted(os.listdir(objdir)):
        if f.endswith(".hip.o"):
            for name, lines in disassemble(os.path.join(objdir, f)).items():
                out.setdefault(name, []).append((f, normalised(lines)))
    return out


def read_renames(args):
    """{old mangled name: new} from --rename OLD=NEW (repeatable) and --rename-file FILE (a pair a line; blank lines and # comments skipped)"""
    pairs = []
    for i, a in enumerate(args):
        if a == "--rename":
            pairs.append(args[i + 1])
        elif a == "--rename-file":
            with open(args[i + 1]) as f:
                pairs += [ln.strip() for ln in f if ln.strip() and not ln.lstrip().startswith("#")]
    renames = {}
    for p in pairs:
        old, eq, new = p.partition("=")
        if not eq or not old or not new or old in renames:
            sys.exit("--rename wants OLD=NEW, every OLD once: %r" % p)
        renames[old] = new
    return renames


def renamed(theirs, renames):
    """the other tree's functions under this tree's names: a renamed function's key, and its name inside its own branch targets"""
    out = {}
    for name, copies in theirs.items():
        new = renames.get(name, name)
        if new in out or (new != name and new in theirs):
            sys.exit("--rename: %s exists there already" % new)
        out[new] = [(obj, [t.replace("<" + name + "+", "<" + new + "+") for t in ins]) for obj, ins in copies] if new != name else copies
    return out


def compare(other, show, renames):
    mine, theirs = functions(BUILD), functions(other)
    unused = sorted(set(renames) - set(theirs))
    if unused:
        sys.exit("--rename: no such function there: " + ", ".join(unused))
    theirs = renamed(theirs, renames)
    for old, new in sorted(renames.items()):
        print("RENAMED  %s  ->  %s" % (old, new))
    gone, new = sorted(set(theirs) - set(mine)), sorted(set(mine) - set(theirs))
    same = differ = 0
    for name in sorted(set(mine) & set(theirs)):
        for obj, ins in mine[name]:
            if any(ins == t for _, t in theirs[name]):
                same += 1
                continue
            differ += 1
            print("DIFFERS  %s  (%s; there: %s)" % (name, obj, ", ".join(o for o, _ in theirs[name])))
            if show:
                print("\n".join(difflib.unified_diff(theirs[name][0][1], ins, "there", "here", lineterm="", n=2)))
    for n in gone:
        print("MISSING here  %s  (there: %s)" % (n, ", ".join(o for o, _ in theirs[n])))
    for n in new:
        print("ONLY here     %s  (%s)" % (n, ", ".join(o for o, _ in mine[n])))
    per = {}
    for v in mine.values():
        for obj, _ in v:
            per[obj] = per.get(obj, 0) + 1
    print("functions per object here: " + ", ".join("%s %d" % (o[:-len(".hip.o")], c) for o, c in sorted(per.items())))
    print("%d names there, %d here (%d renamed); %d missing here, %d only here; %d copies identical, %d differ"
          % (len(theirs), len(mine), len(renames), len(gone), len(new), same, differ))
    return 1 if gone or new or differ else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], "--diff" in sys.argv[3:], read_renames(sys.argv[3:])))
    for name, lines in disassemble(os.path.join(BUILD, sys.argv[1] + ".hip.o")).items():
        if sys.argv[2] in name:
            print("<%s>:\n%s" % (name, "\n".join(lines)))
