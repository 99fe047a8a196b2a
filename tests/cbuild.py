"""TEST INFRASTRUCTURE ONLY -- the one place under tests/ that runs g++ or gcc (tests/gpu_prims/build.py keeps its own hipcc line).
An artefact is rebuilt when a file the compiler read for it has changed: the compiler writes that list itself, beside the artefact
as <artefact>.d, so no build module keeps one by hand."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def deps(out):
    """the files the compiler read for `out`, as its .d file names them (relative to the repository root when they lie in it)"""
    with open(out + ".d") as f:
        rules = f.read().replace("\\\n", " ").splitlines()
    return [d for r in rules for d in r.partition(":")[2].split()]


def stale(out, extra_deps=()):
    try:
        t = os.path.getmtime(out)
        return any(os.path.getmtime(os.path.join(ROOT, d)) > t for d in [*deps(out), *extra_deps])
    except OSError:  # no artefact, no .d, or a file that one of them names is gone
        return True


def compile(out, flags, inputs, compiler="g++", extra_deps=()):
    """`compiler flags -o out inputs`, run at the repository root (sources and -I paths are relative to it, so the recorded paths
    stay true in a copy of the tree), when `out` is stale: see stale().  extra_deps: what the compiler does not see as a source --
    objects and libraries it links, the build module that holds the flags.  -> out"""
    if stale(out, [__file__, *extra_deps]):
        # (into files of this process's own, then renamed: several pytest-xdist workers may find an artefact stale at once, and none
        # of them must load another one's half-written file)
        tmp = "%s.tmp.%d" % (out, os.getpid())
        # DEPENDENCIES_OUTPUT and not -MMD -MF: it leaves system headers out like -MMD, and where one command compiles several
        # sources it adds a rule per source, while every source overwrites the one file -MF names
        env = dict(os.environ, DEPENDENCIES_OUTPUT=tmp + ".d")
        try:
            subprocess.check_call([compiler, *flags, "-o", tmp, *inputs], cwd=ROOT, env=env)
            os.replace(tmp + ".d", out + ".d")
            os.replace(tmp, out)
        finally:
            for f in (tmp, tmp + ".d"):
                if os.path.exists(f):
                    os.unlink(f)
    return out


EMU = ["-pthread", "-Itests/emu"]
SANITIZE = ["-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def emu_lib(out, src, module, defines=()):
    """product kernels on the thread emulator (tests/emu/hip_emu.h) as a shared object that Python loads"""
    return compile(out, ["-std=c++20", "-O1", "-g", "-fPIC", "-shared", *("-D" + d for d in defines), *EMU], [src], extra_deps=[module])


def emu_program(out, src, module, main=None):
    """the same with AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own: nothing sanitized is loaded into
    Python.  main: the macro that turns the driver's main() on, where it has one"""
    return compile(out, ["-std=c++20", "-O1", "-g", *SANITIZE, *(["-D" + main] if main else []), *EMU], [src],
                   extra_deps=[module])


def stand_in(here, srcs, module, emu_src=None, host_lib=None):
    """<here>/libfastplong_amd.so: the sources of a stand-in for the C-ABI library (like every source here, named from the
    repository root), linked with the oracle's C restatement and -- emu_src: (object name, source) -- with product kernels compiled
    for the emulator, or -- host_lib -- against the product's host library and zlib.  As with make, an object that is missing is
    compiled again and the library linked again"""
    objs = [compile(os.path.join(here, "fpl_oracle.o"), ["-O2", "-fPIC", "-c"], ["oracle/fpl_oracle.c"], compiler="gcc")]
    flags, libs = ["-O2", "-std=c++17", "-fPIC", "-shared"], []
    if emu_src:
        objs.append(compile(os.path.join(here, emu_src[0]), ["-std=c++20", "-O1", "-fPIC", *EMU, "-c"], [emu_src[1]]))
        flags.append("-pthread")
    if host_lib:
        d = os.path.dirname(host_lib)
        flags.append("-Iinclude")
        libs = ["-L" + d, "-lfastplong_host", "-Wl,-rpath," + d, "-lz"]
    return compile(os.path.join(here, "libfastplong_amd.so"), flags, [*srcs, *objs, *libs, "-lm"],
                   extra_deps=[*objs, *([host_lib] if host_lib else []), module])
