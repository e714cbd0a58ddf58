"""CPU, text only: include/mink_hip.h says where every entry point lives, and says it truthfully.

Every function the header declares sits under a `/* ---- title (csrc/a.hip, csrc/b.hip)` line.  That title names at least one
csrc/*.hip file, every file it names exists, the function is DEFINED -- its return type and name at column 0, followed by `(`
-- in exactly one .hip file under csrc, and that file is one the title names.  No build, no GPU."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nerf_downstream_amd", "csrc")
RETURNS = r"(?:int|int32_t|int64_t|const char \*)"


def _sections():
    """[(title, files it names, functions declared under it)] in header order."""
    text = open(os.path.join(ROOT, "include", "mink_hip.h")).read()
    titles = [(m.start(), m.group(1).strip()) for m in re.finditer(r"^/\* -{4,}([^\n]*)", text, flags=re.M)]
    code = re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)), text, flags=re.S)  # (offsets kept)
    out = [(t, re.findall(r"\bcsrc/(\w+\.hip)\b", t), []) for _, t in titles]
    for m in re.finditer(rf"^{RETURNS} ?(mink_[a-z0-9_]+)\(", code, flags=re.M):
        above = [i for i, (pos, _) in enumerate(titles) if pos < m.start()]
        assert above, f"{m.group(1)} is declared above the first section title"
        out[above[-1]][2].append(m.group(1))
    return out


def test_every_declaration_sits_under_the_file_that_defines_it():
    sources = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(CSRC, "*.hip"))}
    sections = _sections()
    names = [n for _, _, fs in sections for n in fs]
    assert len(sections) >= 25 and len(names) >= 141 and len(set(names)) == len(names)
    for title, files, funcs in sections:
        for f in files:
            assert f in sources, f"section {title!r} names csrc/{f}, which does not exist"
        for name in funcs:
            assert files, f"{name}: its section {title!r} names no csrc file"
            homes = sorted(f for f, src in sources.items() if re.search(rf"^{RETURNS} ?{name}\(", src, flags=re.M))
            assert len(homes) == 1, f"{name} is defined in {homes or 'no file'}: one definition expected"
            assert homes[0] in files, f"{name} is defined in csrc/{homes[0]}, but declared under {title!r}"


def test_the_split_coordinate_files_are_each_named():
    """The five files that took over csrc/coords.hip's subjects each have their section(s): library state, maps, tables, derived
    orders, the dataset decoder."""
    homes = {f: set() for f in ("lib.hip", "coords.hip", "kmap.hip", "rulebook.hip", "plenoxel.hip")}
    for _, files, funcs in _sections():
        for f in files:
            if f in homes:
                homes[f].update(funcs)
    assert {"mink_last_error", "mink_abi_version"} <= homes["lib.hip"]
    assert {"mink_coords_make_keys", "mink_coords_unique", "mink_coords_build_levels", "mink_batch_offsets"} <= homes["coords.hip"]
    assert {"mink_kernel_map", "mink_kernel_map_batch", "mink_set_overflow_sink"} <= homes["kmap.hip"]
    assert {"mink_rulebook", "mink_class_partition", "mink_class_partition_batch"} <= homes["rulebook.hip"]
    assert homes["plenoxel.hip"] == {"mink_decode_plenoxel"}
