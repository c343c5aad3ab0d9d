"""Asset ingestion: Wavefront OBJ/MTL and glTF 2.0 (.gltf / .glb) -> the triangle / normal / material arrays hr_scene_desc takes
(the layout of scene_descriptor_set.glsl:5-34 after instance flattening), and PNG -> the Heitz-2019 blue-noise tables
(blue_noise.cpp:5-19: ``sobol_256_4d.png`` row 0 and a 128x128 ``scrambling_ranking_128x128_2d_*spp.png``).

The reference loads meshes through assimp and images through stb_image (external/dwSampleFramework, absent here); these
are self-contained readers for the subset those assets use: triangulated or polygonal ``f`` records with v / v/vt / v//vn /
v/vt/vn indices (negative indices allowed), ``usemtl`` + ``mtllib`` (Kd, Pr / Ns, Pm, Ke), ``o`` / ``g`` groups -> mesh ids;
8-bit non-interlaced PNG of colour type 0, 2, 4 or 6 with all five scanline filters; Radiance ``.hdr`` (RGBE, flat or new-style run-length
scanlines, top-down) -> the fp32 equirectangular image env.Environment.update_equirect takes (common.cpp:597-612 loads its four through stbi_loadf).
``load_gltf_skinned`` reads what the static loaders drop — skins, JOINTS_0 / WEIGHTS_0, morph targets and animations — into a SkinnedMesh for
skinning.Skin (include/hr_skin.h).
"""
from __future__ import annotations

import math
import os
import struct
import zlib

import numpy as np

from .synth import SceneData


# ------------------------------------------------------------------------------------------------ OBJ / MTL
def load_mtl(path: str) -> dict:
    """name -> [albedo rgb, metallic, roughness, emissive rgb] (float32[8]).  Pr/Pm are the PBR extension; without Pr the
    Phong exponent maps to roughness = sqrt(2 / (Ns + 2)) (the usual Blinn-Phong -> GGX conversion)."""
    mats, cur, has_pr = {}, None, set()
    with open(path, "r", errors="replace") as f:
        for line in f:
            t = line.split()
            if not t or t[0].startswith("#"):
                continue
            k = t[0].lower()
            if k == "newmtl":
                name = " ".join(t[1:])
                cur = np.array([0.8, 0.8, 0.8, 0.0, 0.5, 0.0, 0.0, 0.0], np.float32)
                mats[name] = cur
            elif cur is None:
                continue
            elif k == "kd":
                cur[0:3] = [float(x) for x in t[1:4]]
            elif k == "pr":
                cur[4] = float(t[1])
                has_pr.add(name)
            elif k == "pm":
                cur[3] = float(t[1])
            elif k == "ns" and name not in has_pr:
                cur[4] = float(np.sqrt(2.0 / (float(t[1]) + 2.0)))
            elif k == "ke":
                cur[5:8] = [float(x) for x in t[1:4]]
    return mats


def load_obj(path: str, scale: float = 1.0, default_material=(0.8, 0.8, 0.8, 0.0, 0.5, 0.0, 0.0, 0.0)) -> SceneData:
    """Triangles in file order; polygons are fanned; missing normals become the geometric face normal (what assimp's
    aiProcess_GenNormals yields for flat faces)."""
    pos, nrm = [], []
    tri_v, tri_n, tri_mat, tri_mesh = [], [], [], []
    mat_names, mat_index, mtl = [], {}, {}
    cur_mat, cur_mesh, n_mesh = None, 1, 1
    base = os.path.dirname(os.path.abspath(path))

    def mat_id(name):
        if name not in mat_index:
            mat_index[name] = len(mat_names)
            mat_names.append(name)
        return mat_index[name]

    with open(path, "r", errors="replace") as f:
        for line in f:
            t = line.split()
            if not t or t[0].startswith("#"):
                continue
            k = t[0]
            if k == "v":
                pos.append([float(t[1]) * scale, float(t[2]) * scale, float(t[3]) * scale])
            elif k == "vn":
                nrm.append([float(t[1]), float(t[2]), float(t[3])])
            elif k == "f":
                idx = []
                for c in t[1:]:
                    p = c.split("/")
                    vi = int(p[0])
                    ni = int(p[2]) if len(p) > 2 and p[2] else 0
                    idx.append((vi - 1 if vi > 0 else len(pos) + vi, (ni - 1 if ni > 0 else len(nrm) + ni) if ni else -1))
                for i in range(1, len(idx) - 1):
                    tri = (idx[0], idx[i], idx[i + 1])
                    tri_v.append([t_[0] for t_ in tri])
                    tri_n.append([t_[1] for t_ in tri])
                    tri_mat.append(mat_id(cur_mat))
                    tri_mesh.append(cur_mesh)
            elif k == "usemtl":
                cur_mat = " ".join(t[1:])
            elif k == "mtllib":
                mp = os.path.join(base, " ".join(t[1:]))
                if os.path.exists(mp):
                    mtl.update(load_mtl(mp))
            elif k in ("o", "g"):
                n_mesh += 1
                cur_mesh = n_mesh
    if not tri_v:
        raise ValueError(f"{path}: no faces")
    P = np.asarray(pos, np.float32)
    verts = P[np.asarray(tri_v, np.int64)]                                  # [n,3,3]
    fn = np.cross(verts[:, 1] - verts[:, 0], verts[:, 2] - verts[:, 0])
    fn = fn / np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-20)
    normals = np.repeat(fn[:, None, :], 3, axis=1).astype(np.float32)
    ni = np.asarray(tri_n, np.int64)
    if len(nrm):
        N = np.asarray(nrm, np.float32)
        has = ni >= 0
        normals[has] = N[ni[has]]
    materials = np.stack([np.asarray(mtl.get(n, default_material), np.float32) for n in mat_names]) if mat_names else np.asarray([default_material], np.float32)
    return SceneData(verts=np.ascontiguousarray(verts), normals=np.ascontiguousarray(normals), tri_material=np.asarray(tri_mat, np.uint32),
                     tri_mesh_id=np.asarray(tri_mesh, np.uint32), materials=np.ascontiguousarray(materials), name=os.path.basename(path),
                     meta=dict(materials=mat_names))


# ------------------------------------------------------------------------------------------------ PNG
_PNG_SIG = b"\x89PNG\r\n\x1a\n"


def load_png(path: str) -> np.ndarray:
    """[H, W, C] uint8 (C = 1, 2, 3 or 4).  8-bit, non-interlaced."""
    return decode_png(open(path, "rb").read(), path)


def decode_png(data: bytes, path: str = "<memory>") -> np.ndarray:
    if data[:8] != _PNG_SIG:
        raise ValueError(f"{path}: not a PNG")
    o, idat, ihdr = 8, [], None
    while o < len(data):
        n, typ = struct.unpack(">I4s", data[o:o + 8])
        body = data[o + 8:o + 8 + n]
        if zlib.crc32(typ + body) & 0xffffffff != struct.unpack(">I", data[o + 8 + n:o + 12 + n])[0]:
            raise ValueError(f"{path}: CRC mismatch in {typ!r}")
        if typ == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif typ == b"IDAT":
            idat.append(body)
        elif typ == b"IEND":
            break
        o += 12 + n
    w, h, depth, ctype, _, _, interlace = ihdr
    if depth != 8 or interlace != 0 or ctype not in (0, 2, 4, 6):
        raise ValueError(f"{path}: only 8-bit non-interlaced grey / RGB / grey+alpha / RGBA PNGs are supported")
    c = {0: 1, 2: 3, 4: 2, 6: 4}[ctype]
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8)
    stride = w * c
    rows = raw.reshape(h, stride + 1)
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.int32)
    for y in range(h):
        ft, line = int(rows[y, 0]), rows[y, 1:].astype(np.int32)
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 255
        elif ft in (1, 3, 4):
            cur = np.zeros(stride, np.int32)
            for i in range(stride):                     # left-dependent filters: sequential along the scanline
                a = cur[i - c] if i >= c else 0
                b = prev[i]
                if ft == 1:
                    p = a
                elif ft == 3:
                    p = (a + b) >> 1
                else:
                    cc = prev[i - c] if i >= c else 0
                    pa, pb, pc = abs(b - cc), abs(a - cc), abs(a + b - 2 * cc)
                    p = a if (pa <= pb and pa <= pc) else (b if pb <= pc else cc)
                cur[i] = (line[i] + p) & 255
        else:
            raise ValueError(f"{path}: bad filter type {ft}")
        out[y] = cur
        prev = cur
    return out.reshape(h, w, c)


def _rgba(img: np.ndarray) -> np.ndarray:
    h, w, c = img.shape
    if c == 4:
        return img
    out = np.full((h, w, 4), 255, np.uint8)
    if c == 1:
        out[..., :3] = img
    elif c == 2:
        out[..., :3] = img[..., :1]; out[..., 3] = img[..., 1]
    else:
        out[..., :3] = img
    return out


def load_blue_noise(sobol_png: str, scrambling_ranking_png: str):
    """(sobol [256,4] uint8, scrambling_ranking [128,128,4] uint8) as hr_frame_inputs takes them: texelFetch(sobol,
    ivec2(i, 0)) reads row 0 only (bnd_sampler.glsl:16), the scrambling/ranking tile is 128x128 RGBA."""
    s, r = _rgba(load_png(sobol_png)), _rgba(load_png(scrambling_ranking_png))
    if s.shape[1] < 256 or r.shape[0] < 128 or r.shape[1] < 128:
        raise ValueError("blue-noise tables must be at least 256 wide (sobol) and 128x128 (scrambling/ranking)")
    return np.ascontiguousarray(s[0, :256]), np.ascontiguousarray(r[:128, :128])


# ------------------------------------------------------------------------------------------------ Radiance .hdr (RGBE)
_HDR_MAX = float(255.0 * 2.0 ** 119)      # the largest RGBE value: mantissa 255 at exponent byte 255


def decode_hdr(data: bytes, path: str = "<memory>") -> np.ndarray:
    """float32 [h, w, 4], alpha 1.  Header ``#?RADIANCE`` or ``#?RGBE``, ``FORMAT=32-bit_rle_rgbe``, a blank line, ``-Y h +X w``; every scanline is flat
    (w RGBE quadruples) or new-style run-length (2, 2, w >> 8, w & 255, then four channel planes of runs; widths 8..32767).  A texel decodes as
    stbi_loadf does: mantissa * 2^(exponent - 136), exponent byte 0 gives 0.  Anything else raises ValueError naming the file and the offset."""
    def fail(what, o):
        raise ValueError(f"{path}: {what} at offset {o}")

    o, lines = 0, []
    while True:                                          # header lines up to the resolution line, which follows the blank line
        nl = data.find(b"\n", o)
        if nl < 0:
            fail("truncated header", o)
        line = data[o:nl]
        lines.append((o, line))
        o = nl + 1
        if len(lines) >= 2 and lines[-2][1] == b"":
            break
    if lines[0][1] not in (b"#?RADIANCE", b"#?RGBE"):
        fail("not a Radiance file (no #?RADIANCE / #?RGBE)", 0)
    formats = [(lo, ln) for lo, ln in lines[1:-2] if ln.startswith(b"FORMAT=")]
    if not formats or formats[0][1] != b"FORMAT=32-bit_rle_rgbe":
        fail("unsupported format (FORMAT=32-bit_rle_rgbe only)", formats[0][0] if formats else lines[0][0])
    ro, res = lines[-1]
    t = res.split()
    if len(t) != 4 or t[0] != b"-Y" or t[2] != b"+X" or not t[1].isdigit() or not t[3].isdigit() or int(t[1]) < 1 or int(t[3]) < 1:
        fail(f"unsupported resolution line {res!r} (-Y h +X w only)", ro)
    h, w = int(t[1]), int(t[3])
    buf = np.frombuffer(data, np.uint8)
    rgbe = np.zeros((h, w, 4), np.uint8)
    for y in range(h):
        rle = 8 <= w <= 32767 and o + 4 <= len(data) and data[o] == 2 and data[o + 1] == 2 and not data[o + 2] & 0x80
        if not rle:
            if o + 4 * w > len(data):
                fail(f"truncated flat scanline {y}", len(data))
            rgbe[y] = buf[o:o + 4 * w].reshape(w, 4)
            o += 4 * w
            continue
        if (data[o + 2] << 8 | data[o + 3]) != w:
            fail(f"scanline {y} is {data[o + 2] << 8 | data[o + 3]} wide, the image {w}", o)
        o += 4
        for c in range(4):
            x = 0
            while x < w:
                if o >= len(data):
                    fail(f"truncated run-length scanline {y}", o)
                n = data[o]
                run = n > 128
                n = n - 128 if run else n
                if n == 0 or n > w - x:
                    fail(f"malformed run of {n} at column {x} of scanline {y}", o)
                if o + 1 + (1 if run else n) > len(data):
                    fail(f"truncated run-length scanline {y}", len(data))
                rgbe[y, x:x + n, c] = data[o + 1] if run else buf[o + 1:o + 1 + n]
                o += 2 if run else 1 + n
                x += n
    e = rgbe[..., 3].astype(np.int32)
    out = np.ones((h, w, 4), np.float32)
    out[..., :3] = rgbe[..., :3].astype(np.float32) * np.where(e > 0, np.ldexp(np.float32(1.0), e - 136), np.float32(0.0)).astype(np.float32)[..., None]
    return out


def load_hdr(path: str) -> np.ndarray:
    """Radiance .hdr -> float32 [h, w, 4] with alpha 1 (decode_hdr)"""
    return decode_hdr(open(path, "rb").read(), path)


def _rle_plane(row: np.ndarray) -> bytes:
    """one channel of a scanline as runs: 128 + n, value for n = 4..127 equal bytes; n, bytes for up to 128 literals"""
    out, w, x, lit = bytearray(), len(row), 0, 0           # lit: start of the pending literals
    b = row.tobytes()
    while x < w:
        n = 1
        while x + n < w and n < 127 and b[x + n] == b[x]:
            n += 1
        if n >= 4:
            while lit < x:
                k = min(128, x - lit)
                out.append(k); out += b[lit:lit + k]
                lit += k
            out.append(128 + n); out.append(b[x])
            x += n
            lit = x
        else:
            x += n
    while lit < w:
        k = min(128, w - lit)
        out.append(k); out += b[lit:lit + k]
        lit += k
    return bytes(out)


def encode_hdr(rgb: np.ndarray, rle: bool = True) -> bytes:
    """[h, w, >= 3] -> the bytes of a Radiance file.  Per texel the shared exponent is that of the largest channel (mantissas truncate, as Ward's
    float2rgbe does), so a value that RGBE can represent is written exactly; below 1e-32 a texel is stored as zeros; negative and NaN channels become 0,
    larger ones the largest RGBE value.  rle: new-style run-length scanlines where the width allows (8..32767), flat otherwise."""
    a = np.asarray(rgb, np.float32)
    if a.ndim != 3 or a.shape[2] < 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("save_hdr: rgb must be [h, w, >= 3]")
    h, w = a.shape[:2]
    c = np.clip(np.nan_to_num(a[..., :3].astype(np.float64), nan=0.0, posinf=_HDR_MAX), 0.0, _HDR_MAX)
    v = c.max(-1)
    _, e = np.frexp(v)
    on = v >= 1e-32
    rgbe = np.zeros((h, w, 4), np.uint8)
    mant = np.floor(c * np.ldexp(1.0, 8 - e)[..., None])
    rgbe[..., :3] = np.where(on[..., None], np.clip(mant, 0, 255), 0).astype(np.uint8)
    rgbe[..., 3] = np.where(on, e + 128, 0).astype(np.uint8)
    out = bytearray(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w))
    for y in range(h):
        if rle and 8 <= w <= 32767:
            out += bytes([2, 2, w >> 8, w & 255])
            for ch in range(4):
                out += _rle_plane(np.ascontiguousarray(rgbe[y, :, ch]))
        else:
            out += rgbe[y].tobytes()
    return bytes(out)


def save_hdr(path: str, rgb: np.ndarray, rle: bool = True) -> None:
    """write [h, w, >= 3] as a Radiance .hdr (encode_hdr)"""
    with open(path, "wb") as f:
        f.write(encode_hdr(rgb, rle))


# ------------------------------------------------------------------------------------------------ glTF 2.0
def _quat_to_mat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float64)


def load_gltf(path: str, scale: float = 1.0, instanced: bool = False):
    """instanced=True: see load_gltf_instanced.  glTF 2.0 (.gltf with external / base64 buffers, or .glb) -> SceneData: the scene's node hierarchy is flattened to world
    space (matrix or TRS nodes), every TRIANGLES primitive contributes its (indexed) triangles, NORMAL is transformed by the
    inverse transpose (missing: geometric normal), materials come from pbrMetallicRoughness (baseColorFactor, metallicFactor,
    roughnessFactor) + emissiveFactor.  One mesh id per (node, primitive).  The reference loads meshes/*.gltf through assimp
    (common.cpp:347-488).  TEXCOORD_0, TANGENT and the PNG images behind baseColorTexture / normalTexture /
    metallicRoughnessTexture (roughness = G, metallic = B) become SceneData.uvs / tangents / material_textures / textures
    (the hit shaders' fetch_* inputs); images in other encodings (JPEG) are skipped, the factor then applies.
    alphaMode MASK fills alpha_cutoffs[m] with alphaCutoff (default 0.5) divided by a baseColorFactor alpha other than 1; OPAQUE and BLEND give 0.
    Nothing applies the array by itself: pass it to Scene.set_alpha_cutoffs.
    emissiveTexture (PNG) fills emissive_textures[m] with an index into `textures` (-1: none), for Scene.set_emissive_textures.  On the device the
    emissive texture REPLACES the emissive constant (include/hr_emission.h), so glTF's "emissiveFactor times emissiveTexture" is honoured here: where
    the factor is not (1, 1, 1) the material gets a COPY of the image whose rgb is round-to-nearest(texel * factor), clipped to 255 (alpha kept); where
    it is (1, 1, 1) the image itself.  materials[m][5..7] stay emissiveFactor: what the material emits if the texture is not bound."""
    import base64
    import json
    raw = open(path, "rb").read()
    base = os.path.dirname(os.path.abspath(path))
    glb_bin = None
    if raw[:4] == b"glTF":
        _, _, total = struct.unpack("<4sII", raw[:12])
        o, doc = 12, None
        while o < total:
            n, typ = struct.unpack("<II", raw[o:o + 8])
            body = raw[o + 8:o + 8 + n]
            if typ == 0x4E4F534A:
                doc = json.loads(body.decode("utf-8"))
            elif typ == 0x004E4942 and glb_bin is None:
                glb_bin = bytes(body)
            o += 8 + n
    else:
        doc = json.loads(raw.decode("utf-8"))
    buffers = []
    for b in doc.get("buffers", []):
        uri = b.get("uri")
        if uri is None:
            buffers.append(glb_bin)
        elif uri.startswith("data:"):
            buffers.append(base64.b64decode(uri.split(",", 1)[1]))
        else:
            buffers.append(open(os.path.join(base, uri), "rb").read())
    comp = {5120: np.int8, 5121: np.uint8, 5122: np.int16, 5123: np.uint16, 5125: np.uint32, 5126: np.float32}
    ncomp = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT4": 16}

    def accessor(i):
        a = doc["accessors"][i]
        dt, nc, cnt = np.dtype(comp[a["componentType"]]), ncomp[a["type"]], a["count"]
        if "bufferView" not in a:
            return np.zeros((cnt, nc), dt)
        bv = doc["bufferViews"][a["bufferView"]]
        off = bv.get("byteOffset", 0) + a.get("byteOffset", 0)
        stride = bv.get("byteStride", 0) or dt.itemsize * nc
        buf = np.frombuffer(buffers[bv["buffer"]], np.uint8)
        rows = np.lib.stride_tricks.as_strided(buf[off:], shape=(cnt, dt.itemsize * nc), strides=(stride, 1))
        return np.ascontiguousarray(rows).view(dt).reshape(cnt, nc)

    textures, image_slot = [], {}

    texture_slot = lambda tex_info: _gltf_texture_slot(doc, buffers, base, textures, image_slot, tex_info)

    mats, mat_tex, cutoffs, em_tex = [], [], [], []
    for m in doc.get("materials", []):
        pbr = m.get("pbrMetallicRoughness", {})
        bc = pbr.get("baseColorFactor", [1, 1, 1, 1])
        em = m.get("emissiveFactor", [0, 0, 0])
        mats.append([bc[0], bc[1], bc[2], pbr.get("metallicFactor", 1.0), pbr.get("roughnessFactor", 1.0), em[0], em[1], em[2]])
        bct, nrm = texture_slot(pbr.get("baseColorTexture")), texture_slot(m.get("normalTexture"))
        mr = texture_slot(pbr.get("metallicRoughnessTexture"))
        mat_tex.append([bct, nrm, mr, mr, 1, 2])
        em_tex.append(_emissive_slot(textures, texture_slot(m.get("emissiveTexture")), em))
        # alphaMode MASK: texel alpha * baseColorFactor alpha < alphaCutoff is cut away; the back end compares the texel alone, so the factor is folded in
        cut = float(m.get("alphaCutoff", 0.5)) if m.get("alphaMode", "OPAQUE") == "MASK" else 0.0
        if cut > 0.0 and float(bc[3]) != 1.0:
            cut = cut / float(bc[3]) if float(bc[3]) > 0.0 else float(np.finfo(np.float32).max)
        cutoffs.append(cut)
    default_mat = len(mats)
    mats.append([0.8, 0.8, 0.8, 0.0, 0.5, 0.0, 0.0, 0.0])
    mat_tex.append([-1, -1, -1, -1, 1, 2])
    cutoffs.append(0.0)
    em_tex.append(-1)

    verts, norms, tmat, tmesh, uvs, tans = [], [], [], [], [], []
    mesh_id = [0]
    node_instances = []   # instanced: (column-major world matrix, glTF mesh index) per node that carries a mesh

    def visit(ni, parent):
        node = doc["nodes"][ni]
        if "matrix" in node:
            local = np.asarray(node["matrix"], np.float64).reshape(4, 4).T
        else:
            local = np.eye(4)
            local[:3, :3] = _quat_to_mat(node.get("rotation", [0, 0, 0, 1])) @ np.diag(node.get("scale", [1, 1, 1]))
            local[:3, 3] = node.get("translation", [0, 0, 0])
        M = parent @ local
        if instanced:
            if "mesh" in node:
                Ms = M.copy()
                Ms[:3, :] *= scale          # world = scale * (M * p)
                node_instances.append((np.ascontiguousarray(Ms.T.reshape(16), np.float32), int(node["mesh"])))
            for c in node.get("children", []):
                visit(c, M)
            return
        if "mesh" in node:
            nm = np.linalg.inv(M[:3, :3]).T
            for prim in doc["meshes"][node["mesh"]]["primitives"]:
                if prim.get("mode", 4) != 4:
                    continue
                pos = accessor(prim["attributes"]["POSITION"]).astype(np.float64)
                idx = accessor(prim["indices"]).reshape(-1).astype(np.int64) if "indices" in prim else np.arange(len(pos))
                idx = idx[: len(idx) // 3 * 3].reshape(-1, 3)
                wp = (pos @ M[:3, :3].T + M[:3, 3]) * scale
                tri = wp[idx]
                if "NORMAL" in prim["attributes"]:
                    n = accessor(prim["attributes"]["NORMAL"]).astype(np.float64) @ nm.T
                    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-20)
                    tn = n[idx]
                else:
                    fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
                    fn /= np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-20)
                    tn = np.repeat(fn[:, None, :], 3, axis=1)
                uv = accessor(prim["attributes"]["TEXCOORD_0"]).astype(np.float32)[idx] if "TEXCOORD_0" in prim["attributes"] else np.zeros((len(tri), 3, 2), np.float32)
                if "TANGENT" in prim["attributes"]:
                    tg = accessor(prim["attributes"]["TANGENT"]).astype(np.float64)[:, :3] @ M[:3, :3].T
                    tg /= np.maximum(np.linalg.norm(tg, axis=1, keepdims=True), 1e-20)
                    tg = tg[idx]
                else:
                    tg = np.zeros_like(tn)
                    tg[..., 0] = 1.0
                uvs.append(uv); tans.append(tg)
                mesh_id[0] += 1
                verts.append(tri); norms.append(tn)
                tmat.append(np.full(len(tri), prim.get("material", default_mat), np.uint32))
                tmesh.append(np.full(len(tri), mesh_id[0], np.uint32))
        for c in node.get("children", []):
            visit(c, M)

    scenes = doc.get("scenes") or [{"nodes": list(range(len(doc.get("nodes", []))))}]
    for root in scenes[doc.get("scene", 0)]["nodes"]:
        visit(root, np.eye(4))
    if instanced:
        from .synth import InstancedSceneData
        # one mesh per glTF mesh (all its TRIANGLES primitives, OBJECT space): scene_descriptor_set.glsl's per-mesh vertex / index / submesh buffers
        used = sorted({k for _, k in node_instances})
        if not used:
            raise ValueError(f"{path}: no node carries a mesh")
        meshes, slot = [], {}
        for k in used:
            mv, mn, mm, mu, mt_ = [], [], [], [], []
            for prim in doc["meshes"][k]["primitives"]:
                if prim.get("mode", 4) != 4:
                    continue
                pos = accessor(prim["attributes"]["POSITION"]).astype(np.float32)
                idx = accessor(prim["indices"]).reshape(-1).astype(np.int64) if "indices" in prim else np.arange(len(pos))
                idx = idx[: len(idx) // 3 * 3].reshape(-1, 3)
                tri = pos[idx]
                if "NORMAL" in prim["attributes"]:
                    tn = accessor(prim["attributes"]["NORMAL"]).astype(np.float32)[idx]
                else:
                    fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).astype(np.float64)
                    fn /= np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-20)
                    tn = np.repeat(fn[:, None, :], 3, axis=1).astype(np.float32)
                mu.append(accessor(prim["attributes"]["TEXCOORD_0"]).astype(np.float32)[idx] if "TEXCOORD_0" in prim["attributes"] else np.zeros((len(tri), 3, 2), np.float32))
                if "TANGENT" in prim["attributes"]:
                    mt_.append(accessor(prim["attributes"]["TANGENT"]).astype(np.float32)[:, :3][idx])
                else:
                    tg = np.zeros_like(tn)
                    tg[..., 0] = 1.0
                    mt_.append(tg)
                mv.append(tri); mn.append(tn)
                mm.append(np.full(len(tri), prim.get("material", default_mat), np.uint32))
            if not mv:
                continue
            slot[k] = len(meshes)
            meshes.append(SceneData(verts=np.ascontiguousarray(np.concatenate(mv), np.float32), normals=np.ascontiguousarray(np.concatenate(mn), np.float32),
                                    tri_material=np.concatenate(mm), tri_mesh_id=np.zeros(sum(len(v) for v in mv), np.uint32), materials=np.asarray(mats, np.float32),
                                    name=doc["meshes"][k].get("name", f"mesh{k}"),
                                    uvs=np.ascontiguousarray(np.concatenate(mu), np.float32) if textures else None,
                                    tangents=np.ascontiguousarray(np.concatenate(mt_), np.float32) if textures else None))
        inst = [(m, slot[k], i + 1) for i, (m, k) in enumerate(node_instances) if k in slot]
        if not inst:
            raise ValueError(f"{path}: no triangle primitives")
        return InstancedSceneData(meshes=meshes, instances=inst, materials=np.asarray(mats, np.float32), name=os.path.basename(path),
                                  material_textures=np.asarray(mat_tex, np.int32) if textures else None, textures=textures if textures else None,
                                  alpha_cutoffs=np.asarray(cutoffs, np.float32), emissive_textures=np.asarray(em_tex, np.int32))
    if not verts:
        raise ValueError(f"{path}: no triangle primitives")
    sd = SceneData(verts=np.ascontiguousarray(np.concatenate(verts), np.float32), normals=np.ascontiguousarray(np.concatenate(norms), np.float32),
                   tri_material=np.concatenate(tmat), tri_mesh_id=np.concatenate(tmesh), materials=np.asarray(mats, np.float32),
                   name=os.path.basename(path), meta=dict(n_materials=len(mats) - 1, n_textures=len(textures)))
    if textures:
        sd.uvs = np.ascontiguousarray(np.concatenate(uvs), np.float32)
        sd.tangents = np.ascontiguousarray(np.concatenate(tans), np.float32)
        sd.material_textures = np.asarray(mat_tex, np.int32)
        sd.textures = textures
    sd.alpha_cutoffs = np.asarray(cutoffs, np.float32)
    sd.emissive_textures = np.asarray(em_tex, np.int32)
    return sd


def _gltf_texture_slot(doc, buffers, base, textures, image_slot, tex_info):
    """glTF textureInfo -> index into `textures`, which grows by the image at its first use (-1: absent or not a PNG)"""
    import base64
    if not tex_info:
        return -1
    src = doc["textures"][tex_info["index"]].get("source")
    if src is None:
        return -1
    if src not in image_slot:
        img, data = doc["images"][src], None
        if "uri" in img:
            data = base64.b64decode(img["uri"].split(",", 1)[1]) if img["uri"].startswith("data:") else open(os.path.join(base, img["uri"]), "rb").read()
        elif "bufferView" in img:
            bv = doc["bufferViews"][img["bufferView"]]
            data = bytes(buffers[bv["buffer"]][bv.get("byteOffset", 0):bv.get("byteOffset", 0) + bv["byteLength"]])
        if data is not None and data[:8] == _PNG_SIG:
            image_slot[src] = len(textures)
            textures.append(np.ascontiguousarray(_rgba(decode_png(data))))
        else:
            image_slot[src] = -1
    return image_slot[src]


def _emissive_slot(textures, slot, factor):
    """the texture a material's emissiveTexture binds: `slot` itself where emissiveFactor is (1, 1, 1), else a copy of it, appended to `textures`,
    whose rgb is the image's times the factor, rounded to nearest and clipped to 255 (load_gltf's docstring); -1 stays -1"""
    f = np.asarray(factor, np.float64)[:3]
    if slot < 0 or np.all(f == 1.0):
        return slot
    t = textures[slot].copy()
    t[..., :3] = np.clip(np.rint(t[..., :3].astype(np.float64) * f), 0, 255).astype(np.uint8)
    textures.append(np.ascontiguousarray(t))
    return len(textures) - 1


def load_gltf_instanced(path: str, scale: float = 1.0):
    """glTF 2.0 -> synth.InstancedSceneData, the layout the reference's scene has on the GPU (scene_descriptor_set.glsl:5-34): one mesh per glTF
    mesh in OBJECT space (positions, normals, texture coordinates, tangents, per-triangle material), one instance { model_matrix, mesh_idx } per
    node that carries a mesh (world matrix of the node hierarchy, times `scale`; mesh id = 1 + the node's order of appearance).  A mesh referenced
    by several nodes is stored once.  hr.InstancedScene(ctx, it) builds it; its flatten() gives the world-space triangles load_gltf() returns
    (up to the rounding of the pinned fp32 transform; normals through mat3(model), as transform_vertex does, not the inverse transpose)."""
    return load_gltf(path, scale, instanced=True)


def load_gltf_lights(path: str, scale: float = 1.0) -> np.ndarray:
    """The KHR_lights_punctual lights of a glTF 2.0 file -> hr_light records, float32 [n, 4, 4] (rows data0 .. data3; what ``Scene.set_lights`` takes),
    one per node of the default scene that carries a light, in the order the hierarchy is visited.  Per record: data0.xyz the node's world +Z axis,
    normalised (a glTF light shines along its node's -Z; data0 points TO the light), data0.w the light's ``intensity`` as written (no unit is
    converted); data1.xyz the node's world translation (times ``scale``, as load_gltf scales positions), radius 0; data2.xyz the ``color``;
    data3 = (0 directional / 1 point / 2 spot, cos(outerConeAngle), cos(innerConeAngle)) with glTF's defaults pi/4 and 0 for a spot and zeros for
    the other types.  ``range`` is IGNORED: the library's lights have no range (include/hr_lights.h).  A file without the extension: [0, 4, 4]."""
    doc, _ = _gltf_document(path)
    defs = doc.get("extensions", {}).get("KHR_lights_punctual", {}).get("lights", [])
    kinds = {"directional": 0.0, "point": 1.0, "spot": 2.0}
    out = []

    def visit(ni, parent):
        node = doc["nodes"][ni]
        if "matrix" in node:
            local = np.asarray(node["matrix"], np.float64).reshape(4, 4).T
        else:
            local = np.eye(4)
            local[:3, :3] = _quat_to_mat(node.get("rotation", [0, 0, 0, 1])) @ np.diag(node.get("scale", [1, 1, 1]))
            local[:3, 3] = node.get("translation", [0, 0, 0])
        M = parent @ local
        ref = node.get("extensions", {}).get("KHR_lights_punctual")
        if ref is not None:
            li = int(ref["light"])
            if not 0 <= li < len(defs):
                raise ValueError(f"{path}: node {ni} names light {li}; the file defines {len(defs)}")
            d = defs[li]
            if d.get("type") not in kinds:
                raise ValueError(f"{path}: light {li} has type {d.get('type')!r}; KHR_lights_punctual knows directional, point and spot")
            z = M[:3, 2]
            zl = float(np.linalg.norm(z))
            if not zl > 0.0:
                raise ValueError(f"{path}: node {ni} has a degenerate transform: its light has no direction")
            rec = np.zeros((4, 4), np.float64)
            rec[0, :3], rec[0, 3] = z / zl, float(d.get("intensity", 1.0))
            rec[1, :3] = M[:3, 3] * scale
            rec[2, :3] = d.get("color", [1.0, 1.0, 1.0])
            rec[3, 0] = kinds[d["type"]]
            if d["type"] == "spot":
                spot = d.get("spot", {})
                rec[3, 1], rec[3, 2] = math.cos(float(spot.get("outerConeAngle", math.pi / 4))), math.cos(float(spot.get("innerConeAngle", 0.0)))
            out.append(rec.astype(np.float32))
        for c in node.get("children", []):
            visit(c, M)

    scenes = doc.get("scenes", [])
    roots = scenes[doc.get("scene", 0)].get("nodes", []) if scenes else range(len(doc.get("nodes", [])))
    for r in roots:
        visit(r, np.eye(4))
    return np.stack(out) if out else np.zeros((0, 4, 4), np.float32)


# ------------------------------------------------------------------------------------------------ glTF 2.0: skins, morph targets, animations
def _gltf_document(path: str):
    """(doc, buffers) of a .gltf (external / base64 buffers) or .glb"""
    import base64
    import json
    raw = open(path, "rb").read()
    base = os.path.dirname(os.path.abspath(path))
    glb_bin, doc = None, None
    if raw[:4] == b"glTF":
        _, _, total = struct.unpack("<4sII", raw[:12])
        o = 12
        while o < total:
            n, typ = struct.unpack("<II", raw[o:o + 8])
            body = raw[o + 8:o + 8 + n]
            if typ == 0x4E4F534A:
                doc = json.loads(body.decode("utf-8"))
            elif typ == 0x004E4942 and glb_bin is None:
                glb_bin = bytes(body)
            o += 8 + n
    else:
        doc = json.loads(raw.decode("utf-8"))
    buffers = []
    for b in doc.get("buffers", []):
        uri = b.get("uri")
        if uri is None:
            buffers.append(glb_bin)
        elif uri.startswith("data:"):
            buffers.append(base64.b64decode(uri.split(",", 1)[1]))
        else:
            buffers.append(open(os.path.join(base, uri), "rb").read())
    return doc, buffers


_GLTF_COMP = {5120: np.int8, 5121: np.uint8, 5122: np.int16, 5123: np.uint16, 5125: np.uint32, 5126: np.float32}
_GLTF_NCOMP = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT4": 16}


def _gltf_accessor(doc, buffers, i, path, as_float: bool = False):
    """accessor i as [count, components]; as_float: float64, integer components de-normalised as glTF specifies (c / max, signed clamped at -1)"""
    a = doc["accessors"][i]
    if "sparse" in a:
        raise ValueError(f"{path}: accessor {i} is sparse: sparse accessors are not supported by load_gltf_skinned")
    dt, nc, cnt = np.dtype(_GLTF_COMP[a["componentType"]]), _GLTF_NCOMP[a["type"]], a["count"]
    if "bufferView" not in a:
        v = np.zeros((cnt, nc), dt)
    else:
        bv = doc["bufferViews"][a["bufferView"]]
        off = bv.get("byteOffset", 0) + a.get("byteOffset", 0)
        stride = bv.get("byteStride", 0) or dt.itemsize * nc
        buf = np.frombuffer(buffers[bv["buffer"]], np.uint8)
        rows = np.lib.stride_tricks.as_strided(buf[off:], shape=(cnt, dt.itemsize * nc), strides=(stride, 1))
        v = np.ascontiguousarray(rows).view(dt).reshape(cnt, nc)
    if not as_float:
        return v
    if dt.kind == "f":
        return v.astype(np.float64)
    top = float(np.iinfo(dt).max)
    return np.maximum(v.astype(np.float64) / top, -1.0) if dt.kind == "i" else v.astype(np.float64) / top


def _slerp(a, b, u):
    """glTF's spherical linear interpolation of unit quaternions (x, y, z, w), along the shorter arc"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = float(np.dot(a, b))
    if d < 0.0:
        b, d = -b, -d
    if d > 0.9995:
        q = a + u * (b - a)
        return q / np.linalg.norm(q)
    th = np.arccos(min(d, 1.0))
    return (np.sin((1.0 - u) * th) * a + np.sin(u * th) * b) / np.sin(th)


class SkinnedMesh:
    """What load_gltf_skinned returns.  ``rest``: SceneData of the skinned mesh in the SKIN's space (positions and normals as stored: the skinned
    node's own transform is ignored, as glTF specifies); ``joints`` [n,3,4] uint16 / ``weights`` [n,3,4] float32 per corner; ``target_positions`` /
    ``target_normals`` [n_targets,n,3,3] (None without targets / when a target lacks NORMAL); ``default_morph_weights``; the skeleton — ``joint_nodes``
    (glTF node per joint), ``parents`` (joint index of the nearest ancestor that is a joint, -1: none), ``node_parent`` / ``node_trs`` (every node's
    parent and rest translation, rotation xyzw, scale; a node given by `matrix` keeps it in ``node_matrix``), ``inverse_bind`` [n_joints,4,4] float64 —
    and ``animations``: name -> list of (node, path, times, values, interpolation).  skinning.Skin(ctx, mesh) takes it as it is."""

    def __init__(self):
        self.rest = None
        self.joints = self.weights = None
        self.n_joints = 0
        self.target_positions = self.target_normals = self.default_morph_weights = None
        self.joint_nodes, self.parents, self.node_parent, self.node_trs, self.node_matrix = [], [], [], [], {}
        self.inverse_bind = None
        self.animations = {}
        self.scale = 1.0
        self.name = "skinned"

    @property
    def n_targets(self) -> int:
        return 0 if self.target_positions is None else int(self.target_positions.shape[0])

    def duration(self, animation) -> float:
        return max([float(ch[2][-1]) for ch in self._channels(animation)] or [0.0])

    def _channels(self, animation):
        if animation is None:
            return []
        if isinstance(animation, int):
            animation = list(self.animations)[animation]
        return self.animations[animation]

    @staticmethod
    def _sample(times, values, interpolation, t, rotation):
        t = min(max(float(t), float(times[0])), float(times[-1]))      # clamped to the track
        if len(times) == 1:
            return values[0]
        k = int(np.clip(np.searchsorted(times, t, side="right") - 1, 0, len(times) - 2))
        if interpolation == "STEP":
            return values[k + 1] if t >= times[k + 1] else values[k]
        u = (t - float(times[k])) / (float(times[k + 1]) - float(times[k]))
        if rotation:
            return _slerp(values[k], values[k + 1], u)
        return values[k] + u * (values[k + 1] - values[k])

    def pose(self, animation=None, t: float = 0.0):
        """(matrices [n_joints,16] float32 column-major, morph weights [n_targets] float32 or None) at time ``t`` of ``animation`` (a name, an index,
        or None: the rest pose): world joint matrix times inverse bind matrix, rows scaled by the loader's ``scale``; the hierarchy in float64;
        LINEAR (slerp for rotations) and STEP samplers; ``t`` clamped to each track."""
        trs = [[np.array(v, np.float64) for v in n] for n in self.node_trs]
        mw = None if self.default_morph_weights is None else np.array(self.default_morph_weights, np.float64)
        animated = set()
        for node, path, times, values, interp in self._channels(animation):
            v = self._sample(times, values, interp, t, path == "rotation")
            if path == "weights":
                mw = np.array(v, np.float64)
            else:
                trs[node][("translation", "rotation", "scale").index(path)] = np.array(v, np.float64)
                animated.add(node)
        world = {}

        def world_of(n):
            if n not in world:
                if n in self.node_matrix and n not in animated:
                    local = self.node_matrix[n]
                else:
                    tr, ro, sc = trs[n]
                    local = np.eye(4)
                    local[:3, :3] = _quat_to_mat(ro) @ np.diag(sc)
                    local[:3, 3] = tr
                p = self.node_parent[n]
                world[n] = local if p < 0 else world_of(p) @ local
            return world[n]

        out = np.zeros((self.n_joints, 16), np.float32)
        for j, n in enumerate(self.joint_nodes):
            M = world_of(n) @ self.inverse_bind[j]
            M = M.copy()
            M[:3, :] *= self.scale
            out[j] = M.T.reshape(16)
        return out, (None if mw is None or self.n_targets == 0 else mw.astype(np.float32))


def load_gltf_skinned(path: str, scale: float = 1.0) -> SkinnedMesh:
    """The first skinned mesh of a glTF 2.0 file (a node with `mesh` and `skin`) as a SkinnedMesh: every TRIANGLES primitive's (indexed) triangles
    expanded to the [n][3][3] corner stream with JOINTS_0 (uint8 / uint16) and WEIGHTS_0 (float or normalised integers; each vertex's four weights
    are normalised to sum 1 in float64 before they are rounded to float32), the morph `targets` (POSITION and NORMAL deltas; mesh.weights as the
    default weights), the skeleton and the animations (LINEAR and STEP).  Raises ValueError, naming the cause, for CUBICSPLINE samplers, JOINTS_1
    (more than four influences) and sparse accessors.  Materials as load_gltf gives them; of their textures only emissiveTexture is read, by load_gltf's
    rule (rest.emissive_textures, rest.textures, rest.uvs from TEXCOORD_0; rest.material_textures names no other texture)."""
    doc, buffers = _gltf_document(path)
    acc = lambda i, as_float=False: _gltf_accessor(doc, buffers, i, path, as_float)
    nodes = doc.get("nodes", [])
    skinned = [i for i, n in enumerate(nodes) if "mesh" in n and "skin" in n]
    if not skinned:
        raise ValueError(f"{path}: no node carries both a mesh and a skin")
    node = nodes[skinned[0]]
    skin, mesh = doc["skins"][node["skin"]], doc["meshes"][node["mesh"]]
    out = SkinnedMesh()
    out.scale, out.name = float(scale), mesh.get("name", os.path.basename(path))
    out.joint_nodes = [int(j) for j in skin["joints"]]
    out.n_joints = len(out.joint_nodes)

    mats = []
    for m in doc.get("materials", []):
        pbr = m.get("pbrMetallicRoughness", {})
        bc, em = pbr.get("baseColorFactor", [1, 1, 1, 1]), m.get("emissiveFactor", [0, 0, 0])
        mats.append([bc[0], bc[1], bc[2], pbr.get("metallicFactor", 1.0), pbr.get("roughnessFactor", 1.0), em[0], em[1], em[2]])
    default_mat = len(mats)
    mats.append([0.8, 0.8, 0.8, 0.0, 0.5, 0.0, 0.0, 0.0])
    # the emissive textures alone (load_gltf's rule: a copy times emissiveFactor where that is not (1, 1, 1)), with TEXCOORD_0 when one is bound
    textures, image_slot, base = [], {}, os.path.dirname(os.path.abspath(path))
    em_tex = [_emissive_slot(textures, _gltf_texture_slot(doc, buffers, base, textures, image_slot, m.get("emissiveTexture")), m.get("emissiveFactor", [0, 0, 0]))
              for m in doc.get("materials", [])] + [-1]

    V, N, J, W, TM, TP, TN, UV = [], [], [], [], [], [], [], []
    normal_deltas = True
    for prim in mesh["primitives"]:
        if prim.get("mode", 4) != 4:
            continue
        at = prim["attributes"]
        if "JOINTS_1" in at or "WEIGHTS_1" in at:
            raise ValueError(f"{path}: JOINTS_1 / WEIGHTS_1: more than four influences per vertex are not supported")
        if "JOINTS_0" not in at or "WEIGHTS_0" not in at:
            raise ValueError(f"{path}: a primitive of the skinned mesh has no JOINTS_0 / WEIGHTS_0")
        pos = acc(at["POSITION"]).astype(np.float32)
        idx = acc(prim["indices"]).reshape(-1).astype(np.int64) if "indices" in prim else np.arange(len(pos))
        idx = idx[: len(idx) // 3 * 3].reshape(-1, 3)
        tri = pos[idx]
        if "NORMAL" in at:
            tn = acc(at["NORMAL"]).astype(np.float32)[idx]
        else:
            fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).astype(np.float64)
            fn /= np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-20)
            tn = np.repeat(fn[:, None, :], 3, axis=1).astype(np.float32)
        jn = acc(at["JOINTS_0"])
        if jn.dtype not in (np.uint8, np.uint16):
            raise ValueError(f"{path}: JOINTS_0 must be unsigned byte or unsigned short")
        w = acc(at["WEIGHTS_0"], as_float=True)
        s = w.sum(1, keepdims=True)
        w = np.where(s > 0.0, w / np.where(s > 0.0, s, 1.0), w)
        V.append(tri); N.append(tn); J.append(jn.astype(np.uint16)[idx]); W.append(w.astype(np.float32)[idx])
        TM.append(np.full(len(tri), prim.get("material", default_mat), np.uint32))
        UV.append(acc(at["TEXCOORD_0"], as_float=True).astype(np.float32)[idx] if "TEXCOORD_0" in at else np.zeros((len(tri), 3, 2), np.float32))
        tp, tnd = [], []
        for tg in prim.get("targets", []):
            tp.append(acc(tg["POSITION"], as_float=True).astype(np.float32)[idx] if "POSITION" in tg else np.zeros_like(tri))
            if "NORMAL" in tg:
                tnd.append(acc(tg["NORMAL"], as_float=True).astype(np.float32)[idx])
            else:
                normal_deltas = False
                tnd.append(np.zeros_like(tri))
        TP.append(tp); TN.append(tnd)
    if not V:
        raise ValueError(f"{path}: the skinned mesh has no triangle primitives")
    n_targets = len(TP[0])
    if any(len(tp) != n_targets for tp in TP):
        raise ValueError(f"{path}: the primitives of the skinned mesh differ in their number of morph targets")
    verts = np.ascontiguousarray(np.concatenate(V), np.float32)
    out.rest = SceneData(verts=verts, normals=np.ascontiguousarray(np.concatenate(N), np.float32), tri_material=np.concatenate(TM),
                         tri_mesh_id=np.ones(len(verts), np.uint32), materials=np.asarray(mats, np.float32), name=out.name,
                         emissive_textures=np.asarray(em_tex, np.int32))
    if textures:
        mt = np.full((len(mats), 6), -1, np.int32)
        mt[:, 4], mt[:, 5] = 1, 2
        out.rest.uvs, out.rest.material_textures, out.rest.textures = np.ascontiguousarray(np.concatenate(UV), np.float32), mt, textures
    out.joints = np.ascontiguousarray(np.concatenate(J), np.uint16)
    out.weights = np.ascontiguousarray(np.concatenate(W), np.float32)
    if n_targets:
        out.target_positions = np.ascontiguousarray(np.stack([np.concatenate([tp[t] for tp in TP]) for t in range(n_targets)]), np.float32)
        if normal_deltas:
            out.target_normals = np.ascontiguousarray(np.stack([np.concatenate([tn[t] for tn in TN]) for t in range(n_targets)]), np.float32)
        out.default_morph_weights = np.asarray(mesh.get("weights", [0.0] * n_targets), np.float32)

    out.node_parent = [-1] * len(nodes)
    for i, n in enumerate(nodes):
        for c in n.get("children", []):
            out.node_parent[c] = i
    for i, n in enumerate(nodes):
        out.node_trs.append([np.asarray(n.get("translation", [0, 0, 0]), np.float64), np.asarray(n.get("rotation", [0, 0, 0, 1]), np.float64),
                             np.asarray(n.get("scale", [1, 1, 1]), np.float64)])
        if "matrix" in n:
            out.node_matrix[i] = np.asarray(n["matrix"], np.float64).reshape(4, 4).T
    joint_of = {n: j for j, n in enumerate(out.joint_nodes)}
    for n in out.joint_nodes:
        p = out.node_parent[n]
        while p >= 0 and p not in joint_of:
            p = out.node_parent[p]
        out.parents.append(joint_of.get(p, -1))
    if "inverseBindMatrices" in skin:
        ibm = acc(skin["inverseBindMatrices"], as_float=True)
        out.inverse_bind = np.ascontiguousarray(ibm.reshape(-1, 4, 4).transpose(0, 2, 1))
    else:
        out.inverse_bind = np.tile(np.eye(4), (out.n_joints, 1, 1))
    if len(out.inverse_bind) != out.n_joints:
        raise ValueError(f"{path}: {len(out.inverse_bind)} inverse bind matrices for {out.n_joints} joints")

    for k, an in enumerate(doc.get("animations", [])):
        channels = []
        for ch in an.get("channels", []):
            sm, target = an["samplers"][ch["sampler"]], ch["target"]
            interp = sm.get("interpolation", "LINEAR")
            if interp == "CUBICSPLINE":
                raise ValueError(f"{path}: animation {an.get('name', k)!r} uses a CUBICSPLINE sampler: only LINEAR and STEP are supported")
            if interp not in ("LINEAR", "STEP"):
                raise ValueError(f"{path}: unknown sampler interpolation {interp!r}")
            if "node" not in target or target["path"] not in ("translation", "rotation", "scale", "weights"):
                continue
            times = acc(sm["input"], as_float=True).reshape(-1)
            values = acc(sm["output"], as_float=True)
            if target["path"] == "weights":
                if target["node"] != skinned[0]:
                    continue
                values = values.reshape(len(times), -1)
            channels.append((int(target["node"]), target["path"], times, values, interp))
        out.animations[an.get("name", f"animation{k}")] = channels
    return out
