"""A draw-list builder with ImDrawList's names, index patterns and command splits (imgui_draw.cpp, v1.90.6), for the UI layer
pass (include/szg/ui_layer.h): what produces the input of pipelines.UILayer.recordDraw without Dear ImGui. No text layout, no
font baking, no anti-aliased fringes (ImDrawListFlags_AntiAliasedFill off): filled rectangles, filled triangles and images.

  DrawList   ImDrawList: VtxBuffer, IdxBuffer (16-bit), CmdBuffer; one ImDrawCmd per texture or clip-rect change
  DrawData   ImDrawData: DisplayPos, DisplaySize, FramebufferScale and the lists; flatten() concatenates them the way
             ImGui_ImplVulkan_RenderDrawData does, with global vertex and index offsets

numpy only: the CPU model of the pass (tests/ui_layer_model.py) consumes the same arrays.
"""
from collections import namedtuple

import numpy as np

# ImDrawVert (imgui.h, default layout): 20 bytes
DRAW_VERT = np.dtype([("pos", np.float32, 2), ("uv", np.float32, 2), ("col", np.uint32)])
assert DRAW_VERT.itemsize == 20

# ImDrawCmd after flatten(): offsets are global
FlatCmd = namedtuple("FlatCmd", "clip_rect texture vtx_offset idx_offset elem_count")
FlatDrawData = namedtuple("FlatDrawData", "display_pos display_size framebuffer_scale vertices indices commands")


def col32(r, g, b, a=255):
    """IM_COL32: bytes R, G, B, A from the least significant."""
    return (int(a) << 24) | (int(b) << 16) | (int(g) << 8) | int(r)


def col32f(r, g, b, a=1.0):
    """ImGui::ColorConvertFloat4ToU32: saturate, * 255 + 0.5, truncate."""
    return col32(*(int(min(max(float(v), 0.0), 1.0) * 255.0 + 0.5) for v in (r, g, b, a)))


class DrawCmd:
    """ImDrawCmd"""

    __slots__ = ("ClipRect", "TextureId", "VtxOffset", "IdxOffset", "ElemCount", "UserCallback")

    def __init__(self, clip, tex, vtx_offset, idx_offset):
        self.ClipRect = tuple(float(v) for v in clip)
        self.TextureId = tex
        self.VtxOffset = int(vtx_offset)
        self.IdxOffset = int(idx_offset)
        self.ElemCount = 0
        self.UserCallback = None

    def header(self):
        return self.ClipRect, self.TextureId, self.VtxOffset


class DrawList:
    """ImDrawList. `texture` is the ImTextureID of the font atlas (what untextured primitives sample) and `uv_white` the
    atlas's TexUvWhitePixel: the UV of an opaque white texel."""

    def __init__(self, texture, uv_white=(0.5, 0.5), clip_rect=(-8192.0, -8192.0, 8192.0, 8192.0)):
        self._pos, self._uv, self._col, self._idx = [], [], [], []
        self._clip_stack = [tuple(float(v) for v in clip_rect)]
        self._tex_stack = [texture]
        self.uv_white = (float(uv_white[0]), float(uv_white[1]))
        self._vtx_current = 0  # ImDrawList::_VtxCurrentIdx: index of the next vertex relative to the command's VtxOffset
        self.CmdBuffer = [DrawCmd(self._clip_stack[-1], texture, 0, 0)]

    # ---- buffers, as ImVector exposes them ----
    @property
    def VtxBuffer(self):
        v = np.zeros(len(self._pos), DRAW_VERT)
        if len(v):
            v["pos"] = np.asarray(self._pos, np.float32)
            v["uv"] = np.asarray(self._uv, np.float32)
            v["col"] = np.asarray(self._col, np.uint32)
        return v

    @property
    def IdxBuffer(self):
        return np.asarray(self._idx, np.uint16)

    # ---- command splits: ImDrawList::_OnChangedClipRect / _OnChangedTextureID / _OnChangedVtxOffset ----
    def _on_changed(self):
        cur = self.CmdBuffer[-1]
        want = (self._clip_stack[-1], self._tex_stack[-1], cur.VtxOffset)
        if cur.header() == want:
            return
        if cur.ElemCount != 0:
            self.CmdBuffer.append(DrawCmd(want[0], want[1], cur.VtxOffset, len(self._idx)))
            return
        # an empty command is rewritten in place, or dropped when the one before it already has the wanted header
        if len(self.CmdBuffer) > 1 and self.CmdBuffer[-2].header() == want:
            self.CmdBuffer.pop()
            return
        cur.ClipRect, cur.TextureId = want[0], want[1]

    def push_clip_rect(self, clip_min, clip_max, intersect_with_current_clip_rect=False):
        """ImDrawList::PushClipRect"""
        c = [float(clip_min[0]), float(clip_min[1]), float(clip_max[0]), float(clip_max[1])]
        if intersect_with_current_clip_rect:
            cur = self._clip_stack[-1]
            c = [max(c[0], cur[0]), max(c[1], cur[1]), min(c[2], cur[2]), min(c[3], cur[3])]
        c[2], c[3] = max(c[0], c[2]), max(c[1], c[3])
        self._clip_stack.append(tuple(c))
        self._on_changed()

    def pop_clip_rect(self):
        if len(self._clip_stack) <= 1:
            raise ValueError("pop_clip_rect without push_clip_rect")
        self._clip_stack.pop()
        self._on_changed()

    def push_texture_id(self, texture):
        self._tex_stack.append(texture)
        self._on_changed()

    def pop_texture_id(self):
        if len(self._tex_stack) <= 1:
            raise ValueError("pop_texture_id without push_texture_id")
        self._tex_stack.pop()
        self._on_changed()

    def _reserve(self, vtx_count):
        """ImDrawList::PrimReserve: with ImGuiBackendFlags_RendererHasVtxOffset a primitive whose indices would leave 16 bits
        starts a command with a new VtxOffset."""
        if self._vtx_current + vtx_count >= (1 << 16):
            cur = self.CmdBuffer[-1]
            offset = len(self._pos)
            if cur.ElemCount != 0:
                self.CmdBuffer.append(DrawCmd(self._clip_stack[-1], self._tex_stack[-1], offset, len(self._idx)))
            else:
                cur.VtxOffset = offset
            self._vtx_current = 0

    def _vert(self, pos, uv, col):
        self._pos.append((float(pos[0]), float(pos[1])))
        self._uv.append((float(uv[0]), float(uv[1])))
        self._col.append(int(col) & 0xFFFFFFFF)

    def _prim_rect_uv(self, a, c, uv_a, uv_c, col):
        """ImDrawList::PrimRectUV: vertices a, (c.x, a.y), c, (a.x, c.y); indices 0 1 2, 0 2 3"""
        self._reserve(4)
        i = self._vtx_current
        self._idx += [i, i + 1, i + 2, i, i + 2, i + 3]
        self._vert(a, uv_a, col)
        self._vert((c[0], a[1]), (uv_c[0], uv_a[1]), col)
        self._vert(c, uv_c, col)
        self._vert((a[0], c[1]), (uv_a[0], uv_c[1]), col)
        self._vtx_current += 4
        self.CmdBuffer[-1].ElemCount += 6

    # ---- primitives ----
    def add_rect_filled(self, p_min, p_max, col):
        """ImDrawList::AddRectFilled without rounding: PrimRect"""
        if (int(col) >> 24) & 0xFF == 0:
            return
        self._prim_rect_uv(p_min, p_max, self.uv_white, self.uv_white, col)

    def add_triangle_filled(self, p1, p2, p3, col):
        """ImDrawList::AddTriangleFilled: PathFillConvex without anti-aliasing, a fan 0 1 2"""
        if (int(col) >> 24) & 0xFF == 0:
            return
        self._reserve(3)
        i = self._vtx_current
        self._idx += [i, i + 1, i + 2]
        for p in (p1, p2, p3):
            self._vert(p, self.uv_white, col)
        self._vtx_current += 3
        self.CmdBuffer[-1].ElemCount += 3

    def add_image(self, texture, p_min, p_max, uv_min=(0.0, 0.0), uv_max=(1.0, 1.0), col=0xFFFFFFFF):
        """ImDrawList::AddImage: PrimRectUV under the image's texture"""
        if (int(col) >> 24) & 0xFF == 0:
            return
        push = texture != self._tex_stack[-1]
        if push:
            self.push_texture_id(texture)
        self._prim_rect_uv(p_min, p_max, uv_min, uv_max, col)
        if push:
            self.pop_texture_id()


class DrawData:
    """ImDrawData"""

    def __init__(self, display_pos=(0.0, 0.0), display_size=(0.0, 0.0), framebuffer_scale=(1.0, 1.0), cmd_lists=()):
        self.DisplayPos = (float(display_pos[0]), float(display_pos[1]))
        self.DisplaySize = (float(display_size[0]), float(display_size[1]))
        self.FramebufferScale = (float(framebuffer_scale[0]), float(framebuffer_scale[1]))
        self.CmdLists = list(cmd_lists)

    @property
    def CmdListsCount(self):
        return len(self.CmdLists)

    def flatten(self):
        """The lists concatenated as ImGui_ImplVulkan_RenderDrawData uploads and draws them: one vertex and one index buffer,
        every command at global_vtx_offset + VtxOffset and global_idx_offset + IdxOffset. Commands with a UserCallback are
        skipped: a callback is not a draw."""
        vertices, indices, commands = [], [], []
        global_vtx = global_idx = 0
        for dl in self.CmdLists:
            vtx, idx = dl.VtxBuffer, dl.IdxBuffer
            for c in dl.CmdBuffer:
                if c.UserCallback is not None:
                    continue
                commands.append(FlatCmd(c.ClipRect, c.TextureId, global_vtx + c.VtxOffset, global_idx + c.IdxOffset, c.ElemCount))
            vertices.append(vtx)
            indices.append(idx)
            global_vtx += len(vtx)
            global_idx += len(idx)
        v = np.concatenate(vertices) if vertices else np.zeros(0, DRAW_VERT)
        i = np.concatenate(indices) if indices else np.zeros(0, np.uint16)
        return FlatDrawData(self.DisplayPos, self.DisplaySize, self.FramebufferScale, v, i, commands)
