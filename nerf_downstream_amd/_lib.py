"""ctypes binding of libmink_hip.so (the C ABI declared in include/mink_hip.h).

There is NO fallback: if the shared library is missing or fails to load, importing the
compute path raises.  ``build()`` compiles it in-tree with hipcc for gfx950.
"""
import ctypes
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MINK_HIP_LIB") or os.path.join(_HERE, "libmink_hip.so")  # (override: A/B builds of the same ABI)
CSRC = os.path.join(_HERE, "csrc")
HEADER = os.path.join(_HERE, os.pardir, "include", "mink_hip.h")  # (where csrc/Makefile takes it from)


class HeaderError(ValueError):
    """The header holds something `parse_header` does not know.  A guessed layout would be device-memory corruption."""


_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
            "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double}
_POINTEES = {"void", "uint8_t"}  # known only behind a pointer
_INT = r"(-?[0-9]+)[uU]?"
_DECLARATOR = re.compile(r"\s*((?:\*\s*(?:const\b\s*)?)*)(\w+)\s*(?:\[\s*([0-9]+)\s*\])?\s*")
_SPACE = re.compile(r"\s*")
_ENUM = re.compile(r"enum\s*\{([^{}]*)\}\s*;")
_STRUCT = re.compile(r"typedef\s+struct\b\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;")
_HOOK = re.compile(r"typedef\s+void\s*\(\s*\*\s*(\w+)\s*\)\s*\(([^()]*)\)\s*;")
_PROTOTYPE = re.compile(r"(const\s+char\s*\*\s*|\w+\s+)(mink_\w+)\s*\(([^()]*)\)\s*;")


def parse_header(text):
    """The C ABI a header declares -> (signatures, structs, hooks, constants).

    Comments and the preprocessor guards are dropped; at file scope exactly four forms are known:
      RET mink_name(ARGS);                  signatures[name] = (restype, argtypes); every pointer argument is c_void_p (call
                                            sites pass data_ptr() ints, None, byref() and ctypes arrays) and so is a hook
      typedef struct [Tag] { ... } MinkX;   structs["X"], a ctypes.Structure with the header's fields in order; a pointer to an
                                            earlier struct is POINTER(that class), every other pointer c_void_p
      typedef void (*MinkXHook)(ARGS);      hooks[name] = CFUNCTYPE(None, ...)
      #define NAME <int>, enum { NAME = <int>, ... };     constants[NAME]
    Anything else, and any type name not known here, raises HeaderError with the offending text."""
    signatures, structs, hooks, constants, by_c_name = {}, {}, {}, {}, {}

    def fail(what, where):
        raise HeaderError(f"mink_hip.h: {what}: {' '.join(where.split())!r}")

    def integer(value, where):
        m = re.fullmatch(rf"{_INT}|\(\s*{_INT}\s*\)", value.strip())
        if not m:
            fail("not an integer constant", where)
        return int(m.group(1) or m.group(2))

    def declare(decl, field):
        """`[const] TYPE declarator, ...` -> [(name, ctypes type)].  Only a struct field (field=True) may be an array, a struct
        by value or a typed pointer to a struct; only a parameter may be a hook."""
        m = re.fullmatch(r"\s*(?:const\s+)?(\w+)\b(.*)", decl, re.S)
        if not m:
            fail("not a declaration", decl)
        out = []
        for d in m.group(2).split(","):
            dm = _DECLARATOR.fullmatch(d)
            if not dm:
                fail("not a named declaration", decl)
            base, stars, count = m.group(1), dm.group(1).count("*"), dm.group(3)
            if stars and (base in _SCALARS or base in _POINTEES or base in by_c_name):
                t = ctypes.POINTER(by_c_name[base]) if field and stars == 1 and base in by_c_name else ctypes.c_void_p
            elif not stars and base in _SCALARS:
                t = _SCALARS[base]
            elif not stars and (base in by_c_name if field else base in hooks):
                t = by_c_name[base] if field else ctypes.c_void_p
            else:
                fail(f"unknown type {base + '*' * stars!r}", decl)
            if count and not field:
                fail("array parameter", decl)
            out.append((dm.group(2), t * int(count) if count else t))
        return out

    def parameters(args):
        if args.strip() == "void":
            return []
        return [declare(a, False)[0][1] for a in args.split(",")]

    # preprocessor lines: the include guard, #include and the extern "C" block go, a #define with a value is a constant
    lines, cplusplus = [], False
    for line in re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S).split("\n"):
        word = line.split()
        if not word or not word[0].startswith("#"):
            lines.append("" if cplusplus else line)
        elif word[0] == "#endif":
            cplusplus = False
        elif word == ["#ifdef", "__cplusplus"]:
            cplusplus = True
        elif word[0] == "#define" and len(word) > 2 and re.fullmatch(r"\w+", word[1]):
            constants[word[1]] = integer(line.split(None, 2)[2], line)
        elif not (word[0] in ("#ifndef", "#include") or (word[0] == "#define" and len(word) == 2)):
            fail("unknown preprocessor line", line)
    body = "\n".join(lines)

    pos = _SPACE.match(body).end()
    while pos < len(body):
        if m := _ENUM.match(body, pos):
            entries = [e.strip() for e in m.group(1).split(",")]
            for e in entries[:-1] if not entries[-1] else entries:
                em = re.fullmatch(r"(\w+)\s*=\s*(.+)", e, re.S)
                if not em:
                    fail("enum entry without a value", e or m.group(0))
                constants[em.group(1)] = integer(em.group(2), e)
        elif m := _STRUCT.match(body, pos):
            c_name = m.group(2)
            if not re.fullmatch(r"Mink\w+", c_name):
                fail("struct name without the Mink prefix", c_name)
            fields = [f for d in m.group(1).split(";") if d.strip() for f in declare(d, True)]
            by_c_name[c_name] = structs[c_name[4:]] = type(c_name[4:], (ctypes.Structure,), {"_fields_": fields, "__doc__": c_name})
        elif m := _HOOK.match(body, pos):
            hooks[m.group(1)] = ctypes.CFUNCTYPE(None, *parameters(m.group(2)))
        elif m := _PROTOTYPE.match(body, pos):
            ret = " ".join(m.group(1).split())
            if ret != "const char *" and ret not in _SCALARS:
                fail(f"unknown return type {ret!r}", m.group(0))
            signatures[m.group(2)] = (ctypes.c_char_p if ret == "const char *" else _SCALARS[ret], parameters(m.group(3)))
        else:
            fail("unrecognised declaration", body[pos:].split(";")[0][:200])
        pos = _SPACE.match(body, m.end()).end()
    return signatures, structs, hooks, constants


def constants(prefix):
    """One family of the header's constants with its prefix stripped: constants("MINK_AUG_")["DROPOUT"] is MINK_AUG_DROPOUT."""
    return {k[len(prefix):]: v for k, v in CONSTANTS.items() if k.startswith(prefix)}


with open(HEADER) as _f:
    SIGNATURES, STRUCTS, _HOOKS, CONSTANTS = parse_header(_f.read())  # name -> (restype, argtypes) | class | hook type | int
globals().update(STRUCTS)  # KernelMapDesc, ConvLayer, NormLayer, Exec, Stem, BasicBlock, LevelMaps, Net, ClassPartitionDesc, TimingEntry, ConvLaunchInfo
STAGE_HOOK, BLOCK_DONE_HOOK = _HOOKS["MinkStageHook"], _HOOKS["MinkBlockDoneHook"]
# the input channels mink_wsconv_fwd stages at a time, its output-channel tile, the row count from which a workgroup owns 256 rows
_WS, _FPS = constants("MINK_WSCONV_"), constants("MINK_FPS_")
WSCONV_CHUNK, WSCONV_COUT_TILE, WSCONV_WIDE_ROWS = _WS["CHUNK"], _WS["COUT_TILE"], _WS["WIDE_ROWS"]
# the scene sizes at which mink_fps_scenes changes where a scene lives, and its status bits
FPS_XYZ_REG_ROWS_SMALL, FPS_XYZ_REG_ROWS, FPS_DIST_REG_ROWS = _FPS["XYZ_REG_ROWS_SMALL"], _FPS["XYZ_REG_ROWS"], _FPS["DIST_REG_ROWS"]
FPS_EMPTY_SCENE, FPS_BAD_START, FPS_SCENE_TOO_LARGE = _FPS["EMPTY_SCENE"], _FPS["BAD_START"], _FPS["SCENE_TOO_LARGE"]


def build(force=False):
    """Compile libmink_hip.so in-tree (hipcc --offload-arch=gfx950)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean"])
    subprocess.check_call(["make", "-C", CSRC, "-j4"])
    return LIB_PATH


_lib = None


class MinkHipError(RuntimeError):
    pass


def lib():
    """Load (once) and return the ctypes handle; raises if the native library is absent or of another ABI version."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MinkHipError(
                f"{LIB_PATH} not found: the HIP backend is mandatory (no CPU fallback). "
                "Build it with `python -c 'import __graft_entry__ as g; g.build()'` or `make -C nerf_downstream_amd/csrc`."
            )
        # One HIP runtime per process: torch ships its own libamdhip64; load it first so that
        # libmink_hip.so (linked against the same soname) binds to that instance instead of
        # bringing /opt/rocm's copy in beside it (two runtimes = "no ROCm-capable device").
        import torch  # noqa: F401

        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if a declared symbol is not exported
            fn.restype, fn.argtypes = res, args
        if L.mink_abi_version() != CONSTANTS["MINK_ABI_VERSION"]:  # (a stale build, or a MINK_HIP_LIB of another checkout)
            raise MinkHipError(
                f"{LIB_PATH} is ABI version {L.mink_abi_version()}, include/mink_hip.h declares {CONSTANTS['MINK_ABI_VERSION']}: "
                "rebuild it from this tree with `make -C nerf_downstream_amd/csrc`."
            )
        # A/B knobs of the launch fusions (scripts/ab_bn.py): MINK_BN_FOLD = fold limit in partial rows, MINK_BN_SMALL = 0 / 1 / 8 / 16
        if os.environ.get("MINK_BN_FOLD"):
            L.mink_bn_set_fold(int(os.environ["MINK_BN_FOLD"]))
        if os.environ.get("MINK_BN_SMALL"):
            L.mink_bn_set_small(int(os.environ["MINK_BN_SMALL"]))
        if os.environ.get("MINK_CONV_PIPELINE"):  # (A/B runs: 0 = two-stage mid-layer kernel, 1 / 2 / 3 = three-stage, see mink_hip.h)
            L.mink_conv_set_pipeline(int(os.environ["MINK_CONV_PIPELINE"]))
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise MinkHipError(f"libmink_hip: {lib().mink_last_error().decode()} (code {rc})")
