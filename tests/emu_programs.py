"""The stand-alone host emulations (tests/emu_*/, rules in tests/emu_kernel.mk), built and run: programs of their own with the
sanitizers compiled in, `program case.bin out.bin`.  Used by the tests that run a kernel's text on the host and by the mutation
audits (tests/mutation_audit.py)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


class BuildFailed(Exception):
    """str(): the compiler's words"""


class Died(Exception):
    """the program did not come back with a result; how: one line for a record, str(): that line and the program's last words"""

    def __init__(self, how, last_words=b""):
        super().__init__(how + "\n" + last_words[-4000:].decode(errors="replace"))
        self.how = how


def build(name, out_dir, **variables):
    """tests/<name> into out_dir -> the program's path.  variables: CSRC, SAN and OPT of tests/emu_kernel.mk, for other than the
    defaults (the library's sources, ASan + UBSan, -O1 -g)"""
    out = os.path.join(str(out_dir), name)
    make = subprocess.run(["make", "-C", os.path.join(HERE, name), "-s", "-B", "OUT=" + out] + ["%s=%s" % v for v in variables.items()],
                          stderr=subprocess.PIPE, text=True)
    if make.returncode != 0:
        raise BuildFailed(make.stderr)
    return out


def run(exe, tmp, write, read, timeout=300):
    """one case through the program at `exe`: write(path) makes the case file in the directory `tmp`, read(path) parses what the
    program wrote -> what `read` returns.  Died when the program does not end, does not return 0 or has something to say (a sanitizer's
    report); the two files are gone afterwards"""
    case, out = os.path.join(str(tmp), "case.bin"), os.path.join(str(tmp), "out.bin")
    try:
        write(case)
        try:
            done = subprocess.run([exe, case, out], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=timeout)
        except subprocess.TimeoutExpired:
            raise Died("does not end")
        if done.returncode != 0:
            raise Died("the program dies (exit status %d)" % done.returncode, done.stderr)
        if done.stderr:
            raise Died("the program complains", done.stderr)
        return read(out)
    finally:
        for path in (case, out):
            if os.path.exists(path):
                os.remove(path)
