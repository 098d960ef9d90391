"""Compare the device code of one kernel between two assembly listings (hipcc --cuda-device-only -S), symbol names and labels apart.

    python tools/kernel_asm_diff.py parent.s this.s track_associate_kernel

Prints the number of instructions on either side and a unified diff of the normalised bodies; exit status 0 when they are identical.
A kernel is found by a substring of its (mangled) name; a template instantiation has a different mangled name than the plain function
it was made from, so the two names may differ:  ... parent.s this.s track_associate_kernel14 track_associate_kernelILb0
"""
import difflib
import re
import sys


def kernel_body(path, name):
    """the instructions of the first function whose symbol contains `name`, labels renumbered in order of appearance and the
    function's own symbol replaced, comments and directives dropped"""
    lines = open(path).read().splitlines()
    start = next((i for i, l in enumerate(lines) if re.match(r"^[A-Za-z_.$][\w.$]*:", l) and name in l.split(":")[0]
                  and not l.startswith(".L")), None)
    if start is None:
        raise SystemExit("%s: no function matching %r" % (path, name))
    symbol = lines[start].split(":")[0]
    body, labels = [], {}
    for l in lines[start + 1:]:
        if l.startswith(".Lfunc_end"):
            break
        l = l.split(";")[0].rstrip()
        if not l.strip() or l.strip().startswith("."):
            m = re.match(r"^(\.L\w+):", l.strip())
            if not m:
                continue
            l = m.group(1) + ":"
        body.append(l.strip().replace(symbol, "KERNEL"))
    for l in body:
        for lab in re.findall(r"\.L\w+", l):
            labels.setdefault(lab, "L%d" % len(labels))
    return [re.sub(r"\.L\w+", lambda m: labels[m.group(0)], l) for l in body]


def main(argv):
    if len(argv) not in (4, 5):
        raise SystemExit(__doc__)
    a, b = kernel_body(argv[1], argv[3]), kernel_body(argv[2], argv[-1])
    diff = list(difflib.unified_diff(a, b, argv[1], argv[2], lineterm="", n=2))
    print("%s: %d lines, %s: %d lines, %s" % (argv[1], len(a), argv[2], len(b), "IDENTICAL" if not diff else "%d diff lines" % len(diff)))
    print("\n".join(diff))
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
