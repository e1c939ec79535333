"""CPU (host-emulated kernels): textures of the mesh RGB-D sensor (activesplat_amd/sensor.py; gs_texture_build_mips, gs_mesh_render_textured) and
the GLB reader.  The checks and where their expected values come from: tests/texture_cases.py.  The same checks run on the MI355X in
tests/test_gpu_mesh_textures.py."""
import json
import struct

import numpy as np
import pytest

from tests import texture_cases as tc


def test_emulated_mip_chains(emu):
    tc.check_mip_chains(emu)


def test_emulated_random_textured_scene(emu):
    tc.check_random_scene(emu)


def test_emulated_cases_worked_by_hand(emu):
    tc.check_worked_by_hand(emu)


def test_emulated_grazing_floor(emu):
    tc.check_grazing(emu)


def test_emulated_identity_with_the_untextured_render(emu):
    tc.check_identity(emu)


def test_emulated_guarded_abi_call_and_refusals(emu):
    tc.check_guarded_abi(emu)


def test_emulated_repeatable_and_texture_order_independent(emu):
    tc.check_repeatable(emu)


def test_emulated_python_validation(emu):
    tc.check_python_validation(emu)


def test_emulated_sensor_and_mapper(emu):
    tc.check_sensor_and_mapper(emu)


# ---- load_glb ---------------------------------------------------------------------------------------------------------------------------------

def _write_glb(path, doc, chunks):
    """chunks: the byte strings of the binary chunk, each at a 4-byte boundary; `doc` gets the one buffer"""
    binary = b"".join(chunks)
    assert len(binary) % 4 == 0
    doc = dict(doc, buffers=[dict(byteLength=len(binary))] + doc.get("buffers", []))
    text = json.dumps(doc).encode()
    text += b" " * (-len(text) % 4)
    body = struct.pack("<II", len(text), 0x4E4F534A) + text + struct.pack("<II", len(binary), 0x004E4942) + binary
    with open(path, "wb") as f:
        f.write(b"glTF" + struct.pack("<II", 2, 12 + len(body)) + body)


def _pad4(b):
    return b + b"\0" * (-len(b) % 4)


def _glb_case(tmp_path):
    import io
    from PIL import Image
    rng = np.random.RandomState(21)
    texels = rng.randint(0, 256, (4, 4, 3)).astype(np.uint8)
    png = io.BytesIO()
    Image.fromarray(np.concatenate([texels, np.full((4, 4, 1), 200, np.uint8)], 2), "RGBA").save(png, format="PNG")       # (the alpha is dropped)
    png = png.getvalue()
    # primitive 0: a textured quad, positions interleaved with uvs at a stride of 20 bytes, uint16 indices
    pos0 = rng.uniform(-1, 1, (4, 3)).astype(np.float32)
    uv0 = rng.uniform(-1, 2, (4, 2)).astype(np.float32)
    idx0 = np.array([0, 1, 2, 0, 2, 3], np.uint16)
    inter = np.concatenate([pos0, uv0], 1).astype("<f4").tobytes()
    # primitive 1: a triangle with COLOR_0 (normalized uint8 x 4) only, uint32 indices
    pos1 = rng.uniform(-1, 1, (3, 3)).astype(np.float32)
    col1 = rng.randint(0, 256, (3, 4)).astype(np.uint8)
    idx1 = np.array([2, 0, 1], np.uint32)
    chunks = [inter, _pad4(idx0.astype("<u2").tobytes()), pos1.astype("<f4").tobytes(), col1.tobytes(), idx1.astype("<u4").tobytes(), _pad4(png)]
    offsets = np.cumsum([0] + [len(c) for c in chunks]).tolist()
    views = [dict(buffer=0, byteOffset=offsets[0], byteLength=len(inter), byteStride=20),
             dict(buffer=0, byteOffset=offsets[1], byteLength=12),
             dict(buffer=0, byteOffset=offsets[2], byteLength=36),
             dict(buffer=0, byteOffset=offsets[3], byteLength=12),
             dict(buffer=0, byteOffset=offsets[4], byteLength=12),
             dict(buffer=0, byteOffset=offsets[5], byteLength=len(png))]
    accessors = [dict(bufferView=0, componentType=5126, count=4, type="VEC3"),
                 dict(bufferView=0, byteOffset=12, componentType=5126, count=4, type="VEC2"),
                 dict(bufferView=1, componentType=5123, count=6, type="SCALAR"),
                 dict(bufferView=2, componentType=5126, count=3, type="VEC3"),
                 dict(bufferView=3, componentType=5121, count=3, type="VEC4", normalized=True),
                 dict(bufferView=4, componentType=5125, count=3, type="SCALAR")]
    # the mesh hangs under a translated parent and a rotated (and scaled) child
    angle = 0.7
    quat = [0.0, np.sin(angle / 2), 0.0, np.cos(angle / 2)]                                   # about y
    doc = dict(asset=dict(version="2.0"), scene=0, scenes=[dict(nodes=[0])],
               nodes=[dict(translation=[1.0, -2.0, 0.5], children=[1]), dict(rotation=quat, scale=[2.0, 1.0, 0.5], mesh=0)],
               meshes=[dict(primitives=[dict(attributes=dict(POSITION=0, TEXCOORD_0=1), indices=2, material=0),
                                        dict(attributes=dict(POSITION=3, COLOR_0=4), indices=5, material=1)])],
               materials=[dict(pbrMetallicRoughness=dict(baseColorTexture=dict(index=0))), dict(pbrMetallicRoughness=dict(baseColorFactor=[1, 1, 1, 1]))],
               textures=[dict(source=0, sampler=0)], samplers=[dict(wrapS=33071, wrapT=33648)], images=[dict(bufferView=5, mimeType="image/png")],
               bufferViews=views, accessors=accessors)
    path = str(tmp_path / "scene.glb")
    _write_glb(path, doc, chunks)
    rot = np.array([[np.cos(angle), 0, np.sin(angle)], [0, 1, 0], [-np.sin(angle), 0, np.cos(angle)]])
    world = lambda p: (p.astype(np.float64) * np.array([2.0, 1.0, 0.5])) @ rot.T + np.array([1.0, -2.0, 0.5])  # noqa: E731
    want = dict(vertices=np.concatenate([world(pos0), world(pos1)]), triangles=np.array([[0, 1, 2], [0, 2, 3], [6, 4, 5]], np.int32),
                vertex_colors=np.concatenate([np.full((4, 3), 128, np.uint8), col1[:, :3]]), uvs=np.concatenate([uv0, np.zeros((3, 2), np.float32)]),
                tri_texture=np.array([0, 0, -1], np.int32), texels=texels)
    return path, doc, chunks, want


def test_load_glb(emu, tmp_path):
    pytest.importorskip("PIL")
    from activesplat_amd import sensor as S
    path, doc, chunks, want = _glb_case(tmp_path)
    host = S.read_glb(path)
    scene = S.load_glb(path, device=emu)
    for got in (host, dict(vertices=scene.vertices.numpy(), triangles=scene.triangles.numpy(), vertex_colors=scene.vertex_colors.numpy(),
                           uvs=scene.uvs.numpy(), tri_texture=scene.tri_texture.numpy())):
        assert got["vertices"].dtype == np.float32 and np.abs(got["vertices"] - want["vertices"]).max() <= 1e-6
        assert got["triangles"].dtype == np.int32 and np.array_equal(got["triangles"], want["triangles"])
        assert np.array_equal(got["vertex_colors"], want["vertex_colors"]) and got["vertex_colors"].dtype == np.uint8
        assert np.array_equal(got["uvs"], want["uvs"]) and np.array_equal(got["tri_texture"], want["tri_texture"])
    assert len(host["textures"]) == 1 and np.array_equal(host["textures"][0][0], want["texels"]) and host["textures"][0][1:] == (S.WRAP_CLAMP, S.WRAP_MIRROR)
    assert scene.num_textures == 1 and np.array_equal(scene.texture_level(0, 0).numpy(), want["texels"])
    assert (scene._h_table[0].wrap_s, scene._h_table[0].wrap_t) == (S.WRAP_CLAMP, S.WRAP_MIRROR)
    # the same node transform given as a matrix (column-major)
    m = np.eye(4)
    angle = 0.7
    rot = np.array([[np.cos(angle), 0, np.sin(angle)], [0, 1, 0], [-np.sin(angle), 0, np.cos(angle)]])
    m[:3, :3] = rot * np.array([2.0, 1.0, 0.5])[None, :]
    as_matrix = dict(doc, nodes=[doc["nodes"][0], dict(matrix=m.T.reshape(-1).tolist(), mesh=0)])
    _write_glb(str(tmp_path / "matrix.glb"), as_matrix, chunks)
    assert np.abs(S.read_glb(str(tmp_path / "matrix.glb"))["vertices"] - want["vertices"]).max() <= 1e-6
    # a scene without a textured material has no texture arguments
    bare = dict(doc, materials=[dict(), dict()])
    _write_glb(str(tmp_path / "bare.glb"), bare, chunks)
    host = S.read_glb(str(tmp_path / "bare.glb"))
    assert host["textures"] is None and host["uvs"] is None and host["tri_texture"] is None and S.load_glb(str(tmp_path / "bare.glb"), device=emu).num_textures == 0
    # what is not read raises, naming it
    for change, error, text in ((dict(buffers=[dict(byteLength=4, uri="far.bin")], bufferViews=[dict(doc["bufferViews"][0], buffer=1)] + doc["bufferViews"][1:]),
                                 NotImplementedError, "external buffer"),
                                (dict(extensionsRequired=["KHR_draco_mesh_compression"]), NotImplementedError, "KHR_draco_mesh_compression"),
                                (dict(meshes=[dict(primitives=[dict(doc["meshes"][0]["primitives"][0], extensions=dict(KHR_draco_mesh_compression=dict()))])]),
                                 NotImplementedError, "KHR_draco_mesh_compression"),
                                (dict(meshes=[dict(primitives=[dict(doc["meshes"][0]["primitives"][0], mode=5)])]), NotImplementedError, "mode 5"),
                                (dict(accessors=[dict(doc["accessors"][0], sparse=dict(count=1))] + doc["accessors"][1:]), NotImplementedError, "sparse"),
                                (dict(images=[dict(uri="wall.png")]), NotImplementedError, "external image")):
        _write_glb(str(tmp_path / "bad.glb"), dict(doc, **change), chunks)
        with pytest.raises(error, match=text):
            S.read_glb(str(tmp_path / "bad.glb"))
    with open(str(tmp_path / "not.glb"), "wb") as f:
        f.write(b"glTX" + bytes(20))
    with pytest.raises(ValueError, match="not a GLB"):
        S.read_glb(str(tmp_path / "not.glb"))
