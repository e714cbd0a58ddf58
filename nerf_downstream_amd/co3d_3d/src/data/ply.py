"""PLY reader for the ScanNet point clouds (counterpart of the reference's co3d_3d/src/data/utils.py:8-22 `load_ply`, which
uses the `plyfile` package).  numpy only; like safe_load.py it executes nothing from the file: the header is parsed as
plain text and the body is read as numbers.

Formats: ascii, binary_little_endian, binary_big_endian.  Scalar types under their old and new names (char/int8,
uchar/uint8, short/int16, ushort/uint16, int/int32, uint/uint32, float/float32, double/float64).  The `vertex` element gives
x y z (float32), red green blue (float32) and label (int32).  Elements after `vertex` (faces, edges...) are not read.  An
element before `vertex` is skipped when all its properties are scalars; a list property there (whose size depends on the
data) is refused."""
import numpy as np

_TYPES = {
    "char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
    "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8",
}
_FORMATS = {"ascii": None, "binary_little_endian": "<", "binary_big_endian": ">"}


class PlyError(ValueError):
    pass


def _scalar(name, path):
    if name not in _TYPES:
        raise PlyError(f"{path}: unknown PLY type {name!r}")
    return _TYPES[name]


def read_header(f, path="<ply>"):
    """-> (format, [(element name, count, [(property name, dtype code or ("list", count code, item code))])]), file at the body."""
    if f.readline().strip() != b"ply":
        raise PlyError(f"{path}: not a PLY file")
    fmt, elements = None, []
    while True:
        line = f.readline()
        if not line:
            raise PlyError(f"{path}: header without end_header")
        words = line.decode("ascii", "strict").split()
        if not words or words[0] in ("comment", "obj_info"):
            continue
        if words[0] == "end_header":
            break
        if words[0] == "format":
            if len(words) != 3 or words[1] not in _FORMATS:
                raise PlyError(f"{path}: unsupported format line {line!r}")
            fmt = words[1]
        elif words[0] == "element":
            if len(words) != 3 or int(words[2]) < 0:
                raise PlyError(f"{path}: bad element line {line!r}")
            elements.append((words[1], int(words[2]), []))
        elif words[0] == "property":
            if not elements:
                raise PlyError(f"{path}: property before any element")
            if words[1] == "list":
                if len(words) != 5:
                    raise PlyError(f"{path}: bad list property {line!r}")
                elements[-1][2].append((words[4], ("list", _scalar(words[2], path), _scalar(words[3], path))))
            else:
                if len(words) != 3:
                    raise PlyError(f"{path}: bad property {line!r}")
                elements[-1][2].append((words[2], _scalar(words[1], path)))
        else:
            raise PlyError(f"{path}: unknown header line {line!r}")
    if fmt is None:
        raise PlyError(f"{path}: no format line")
    return fmt, elements


def read_vertices(path):
    """-> dict property name -> numpy array [count] of the `vertex` element, in its stored type."""
    with open(path, "rb") as f:
        fmt, elements = read_header(f, path)
        order = _FORMATS[fmt]
        for name, count, props in elements:
            if any(isinstance(t, tuple) for _, t in props):
                if name == "vertex":
                    raise PlyError(f"{path}: list property in the vertex element")
                raise PlyError(f"{path}: element {name!r} before 'vertex' has a list property: its size cannot be known "
                               "without parsing it")
            if fmt == "ascii":
                rows = []
                for _ in range(count):
                    line = f.readline()
                    if not line:
                        raise PlyError(f"{path}: element {name!r} ends early")
                    rows.append(line.split())
                if name != "vertex":
                    continue
                if any(len(r) < len(props) for r in rows):
                    raise PlyError(f"{path}: a vertex line has fewer than {len(props)} values")
                cols = list(zip(*rows)) if rows else [()] * len(props)
                return {p: np.array([float(v) if t[0] == "f" else int(v) for v in col], dtype=t) for (p, t), col in zip(props, cols)}
            dt = np.dtype([(p, order + t) for p, t in props])
            if name != "vertex":
                f.seek(dt.itemsize * count, 1)
                continue
            buf = f.read(dt.itemsize * count)
            if len(buf) != dt.itemsize * count:
                raise PlyError(f"{path}: vertex data ends early ({len(buf)} of {dt.itemsize * count} bytes)")
            data = np.frombuffer(buf, dtype=dt, count=count)
            return {p: data[p].astype(data[p].dtype.newbyteorder("=")) for p, _ in props}
    raise PlyError(f"{path}: no vertex element")


def load_ply(path, load_label=True):
    """-> (xyz float32 [N,3], colours float32 [N,3], labels int32 [N]) as the reference's load_ply (instances are not read)."""
    v = read_vertices(path)
    need = ["x", "y", "z", "red", "green", "blue"] + (["label"] if load_label else [])
    missing = [p for p in need if p not in v]
    if missing:
        raise PlyError(f"{path}: vertex element without {missing}")
    xyz = np.stack([v["x"], v["y"], v["z"]], 1).astype(np.float32)
    rgb = np.stack([v["red"], v["green"], v["blue"]], 1).astype(np.float32)
    labels = v["label"].astype(np.int32) if load_label else np.zeros(len(xyz), np.int32)
    return xyz, rgb, labels


def write_ply(path, columns, fmt="binary_little_endian", extra_elements=()):
    """Write a PLY file with one `vertex` element: columns = [(name, numpy array [N] whose dtype gives the type)], then
    `extra_elements` = [(name, count, header property lines, raw body bytes)] (test fixtures: faces)."""
    rev = {np.dtype(v).str[1:]: k for k, v in _TYPES.items() if not k[-1].isdigit()}
    n = len(columns[0][1])
    head = ["ply", f"format {fmt} 1.0", f"element vertex {n}"]
    head += [f"property {rev[np.asarray(a).dtype.str[1:]]} {name}" for name, a in columns]
    for name, count, props, _ in extra_elements:
        head += [f"element {name} {count}"] + list(props)
    head.append("end_header")
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if fmt == "ascii":
            for i in range(n):
                f.write((" ".join(repr(a[i].item()) for _, a in columns) + "\n").encode("ascii"))
        else:
            order = _FORMATS[fmt]
            dt = np.dtype([(name, order + np.asarray(a).dtype.str[1:]) for name, a in columns])
            rec = np.empty(n, dt)
            for name, a in columns:
                rec[name] = a
            f.write(rec.tobytes())
        for _, _, _, body in extra_elements:
            f.write(body)
