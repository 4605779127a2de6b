#!/usr/bin/env python3
"""Two assembly files of the same translation unit, function by function: is every function of the first one unchanged in the second?

  python scripts/isa_compare_kernels.py <other.s> <this.s>

For scripts/isa_compare.sh, when a file differs as a whole because this tree ADDS kernels to it.  The numbers that the compiler gives
to a function's labels (.LBB<function>_<block>, the loop comments) count the functions in front of it and are left out.  Prints the
functions that differ or are missing and a summary line; exit status 1 if there is one."""
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
        elif name is not None:
            if re.match(r"^\.Lfunc_end\d+:", line):
                out[name], name = "".join(body), None
            else:
                body.append(line)
    return out


def normalised(text):
    text = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", text)
    return re.sub(r"Header=BB\d+_", "Header=BB_", text)


def main():
    other, this = functions(sys.argv[1]), functions(sys.argv[2])
    bad = 0
    for name, text in other.items():
        if name not in this:
            print("    missing here: %s" % name); bad += 1
        elif normalised(text) != normalised(this[name]):
            print("    differs: %s" % name); bad += 1
    print("    functions of the other tree: %d, identical here: %d, new here: %d" % (len(other), len(other) - bad, len(set(this) - set(other))))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
