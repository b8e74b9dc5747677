"""save_ply on CPU tensors: the header it writes, and the payload read back with NumPy equals the
tensors -- with and without normals, and for the empty mesh."""
import numpy as np
import pytest
import torch


def read_ply(path):
    """-> (vertex rows [V, 3 or 6] float32, triangles [T, 3] int32, header lines)"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[-1] == "end_header"
    elements, props = [], {}
    for line in lines[2:-1]:
        tok = line.split()
        if tok[0] == "element":
            elements.append((tok[1], int(tok[2])))
            props[tok[1]] = []
        elif tok[0] == "property":
            props[elements[-1][0]].append(tok[1:])
        else:
            assert tok[0] == "comment", line
    assert [e[0] for e in elements] == ["vertex", "face"]
    V, T = elements[0][1], elements[1][1]
    assert all(p[0] == "float" for p in props["vertex"])
    names = [p[1] for p in props["vertex"]]
    assert names in (["x", "y", "z"], ["x", "y", "z", "nx", "ny", "nz"])
    assert props["face"] == [["list", "uchar", "int", "vertex_indices"]]
    body = raw[end:]
    nv = 4 * len(names) * V
    assert len(body) == nv + 13 * T
    rows = np.frombuffer(body[:nv], dtype="<f4").reshape(V, len(names))
    faces = np.frombuffer(body[nv:], dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    assert (faces["n"] == 3).all()
    return rows, faces["v"].reshape(T, 3), lines


@pytest.mark.parametrize("with_normals", [False, True], ids=["plain", "normals"])
@pytest.mark.parametrize("V,T", [(7, 5), (1, 1), (0, 0)], ids=["mesh", "one", "empty"])
def test_ply_reads_back(pkg, tmp_path, V, T, with_normals):
    H = pkg.load_host()
    g = torch.Generator().manual_seed(V + 10 * T)
    vertices = torch.randn(V, 3, generator=g)
    triangles = torch.randint(0, max(V, 1), (T, 3), generator=g, dtype=torch.int32)
    normals = torch.randn(V, 3, generator=g) if with_normals else None
    if V:
        vertices[0, 0] = float("nan")                     # bits, not numbers, go to the file
    path = str(tmp_path / "mesh.ply")
    H.save_ply(path, vertices, triangles, normals)
    rows, tri, _ = read_ply(path)
    want = vertices if normals is None else torch.cat([vertices, normals], 1)
    assert rows.shape == tuple(want.shape)
    assert np.array_equal(rows.view(np.int32), want.numpy().view(np.int32))
    assert np.array_equal(tri, triangles.numpy())


def test_ply_takes_views_and_refuses_other_types(pkg, tmp_path):
    H = pkg.load_host()
    path = str(tmp_path / "mesh.ply")
    base = torch.arange(24, dtype=torch.float32).reshape(4, 6)
    vertices, normals = base[:, :3], base[:, 3:]          # not contiguous
    triangles = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32)
    H.save_ply(path, vertices, triangles, normals)
    rows, tri, _ = read_ply(path)
    assert np.array_equal(rows, base.numpy()) and np.array_equal(tri, triangles.numpy())
    with pytest.raises(RuntimeError, match="int32"):
        H.save_ply(path, vertices, triangles.long())
    with pytest.raises(RuntimeError, match="float32"):
        H.save_ply(path, vertices.double(), triangles)
    with pytest.raises(RuntimeError, match="normals"):
        H.save_ply(path, vertices, triangles, normals[:2])
    with pytest.raises(RuntimeError, match="cannot open"):
        H.save_ply(str(tmp_path / "missing" / "mesh.ply"), vertices, triangles)
