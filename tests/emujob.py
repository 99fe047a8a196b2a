"""TEST INFRASTRUCTURE ONLY -- one job of a sanitized program (tests/cbuild.py builds them): the job goes in as the file "in" of a
directory of its own and the result comes out as "out" beside it; the program is started as `exe in out`."""
import os
import struct
import subprocess
import tempfile

ASAN_OPTIONS = "detect_leaks=0:detect_stack_use_after_return=0:abort_on_error=0"


def _clean(d):
    for f in ("in", "out"):
        try:
            os.unlink(os.path.join(d, f))
        except OSError:
            pass
    os.rmdir(d)


def start(exe, payload_writer, prefix, asan_options=ASAN_OPTIONS):
    """payload_writer(f) writes the job; -> a running process, side by side with any other; finish() collects it"""
    d = tempfile.mkdtemp(prefix=prefix)
    try:
        with open(os.path.join(d, "in"), "wb") as f:
            payload_writer(f)
        env = dict(os.environ, ASAN_OPTIONS=asan_options, UBSAN_OPTIONS="print_stacktrace=1")
        return subprocess.Popen([exe, os.path.join(d, "in"), os.path.join(d, "out")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                env=env), d
    except BaseException:
        _clean(d)
        raise


def finish(job, timeout=None):
    """-> the bytes of "out"; raises with the sanitizers' report when the run did not end clean"""
    p, d = job
    try:
        try:
            log = p.communicate(timeout=timeout)[0]
        except subprocess.TimeoutExpired:
            p.kill()
            p.communicate()
            raise
        if p.returncode != 0:
            raise RuntimeError("%s ended with %d:\n%s" % (os.path.basename(p.args[0]), p.returncode, log.decode(errors="replace")[-4000:]))
        with open(os.path.join(d, "out"), "rb") as f:
            return f.read()
    finally:
        _clean(d)


def run(exe, payload_writer, prefix, asan_options=ASAN_OPTIONS, timeout=None):
    return finish(start(exe, payload_writer, prefix, asan_options), timeout)


def write_context_op(f, op):
    """the operations that the walk programs (tests/emu_bamwalk, tests/emu_textwalk) share: 0 new context, 2 tail out, 3 tail in,
    4 resume, 5 tail capacity -> whether op was one of them"""
    if op[0] == "new":
        f.write(struct.pack("<QQ", 0, op[1]))
    elif op[0] == "tail_get":
        f.write(struct.pack("<Q", 2))
    elif op[0] == "tail_set":
        f.write(struct.pack("<QQ", 3, len(op[1])) + bytes(op[1]))
    elif op[0] == "resume":
        f.write(struct.pack("<Q", 4))
    elif op[0] == "reserve":
        f.write(struct.pack("<QQ", 5, op[1]))
    else:
        return False
    return True
