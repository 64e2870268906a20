"""What the GPU tests of the UI layer pass share (tests/test_gpu_ui_layer.py and its child process
tests/gpu_ui_layer_child.py): a szg_ui_layer driven through the C-ABI with the inputs of the CPU model, and a padded target
filled with a sentinel."""
import ctypes as C

import numpy as np

from syzygy_amd import abi, lib
from tests import ui_layer_model as um

BLACK = (0.0, 0.0, 0.0, 1.0)


def to_device(torch, array):
    raw = np.frombuffer(np.ascontiguousarray(array).tobytes() or b"\0", np.uint8).copy()
    return torch.from_numpy(raw).cuda()


class Target:
    """An RGBA16_UNORM image of iw x ih texels inside a buffer whose rows carry `pad` more texels (pitch padding) and which has
    two more rows than the image, all filled with a sentinel pattern. The WHOLE buffer is compared."""

    def __init__(self, torch, iw, ih, pad=3, seed=1):
        rng = np.random.default_rng(seed)
        self.torch, self.iw, self.ih, self.pad = torch, iw, ih, pad
        self.buffer0 = rng.integers(0, 65536, (ih + 2, iw + pad, 4), dtype=np.uint16)
        self.reset()

    def reset(self, image=None):
        if image is not None:
            self.buffer0 = self.buffer0.copy()
            self.buffer0[:self.ih, :self.iw] = image
        self.buffer = self.torch.from_numpy(self.buffer0.view(np.int16).copy()).cuda()

    @property
    def image0(self):
        return self.buffer0[:self.ih, :self.iw]

    def abi(self):
        return abi.Image(self.buffer.data_ptr(), self.iw, self.ih, (self.iw + self.pad) * 8, abi.SZG_FORMAT_RGBA16_UNORM)

    def read(self):
        self.torch.cuda.synchronize()
        return self.buffer.cpu().numpy().view(np.uint16)

    def expect(self, image):
        out = self.buffer0.copy()
        out[:self.ih, :self.iw] = image
        return out


class Layer:
    def __init__(self, torch, triangle_capacity=1 << 15, command_capacity=256):
        self.torch = torch
        self.h = C.c_void_p()
        assert lib().szg_ui_layer_create(C.byref(self.h), triangle_capacity, command_capacity, 0) == abi.SZG_OK, lib().szg_last_error()
        self.keep = []

    def destroy(self):
        if self.h:
            lib().szg_ui_layer_destroy(self.h)
            self.h = None

    def add_texture(self, tex, pitch_pad=0):
        """um.Texture -> handle. pitch_pad: extra texels per row of the device copy."""
        data = tex.data
        h, w = data.shape[:2]
        padded = np.zeros((h, w + pitch_pad, 4), data.dtype)
        padded[:, :w] = data
        fmt = abi.SZG_FORMAT_RGBA16_UNORM if data.dtype == np.uint16 else abi.SZG_FORMAT_RGBA8_UNORM
        d = to_device(self.torch, padded)
        im = abi.Image(d.data_ptr(), w, h, (w + pitch_pad) * data.dtype.itemsize * 4, fmt)
        out = C.c_void_p()
        rc = lib().szg_ui_layer_add_texture(self.h, C.byref(im), abi.UISampler(tex.filter, tex.address), C.byref(out))
        assert rc == abi.SZG_OK, lib().szg_last_error()
        self.keep.append(d)
        return out.value

    def remove_texture(self, handle):
        return lib().szg_ui_layer_remove_texture(self.h, C.c_void_p(handle))

    def draw_data(self, draw, handles):
        """(abi.UIDrawData, what must stay alive) for a ui.FlatDrawData whose commands name keys of `handles`"""
        d_v, d_i = to_device(self.torch, draw.vertices), to_device(self.torch, np.asarray(draw.indices, np.uint16))
        n = len(draw.commands)
        commands = (abi.UIDrawCmd * max(n, 1))()
        for dst, c in zip(commands, draw.commands):
            dst.clip_rect[:] = [float(v) for v in c.clip_rect]
            dst.texture = handles.get(c.texture, c.texture) if c.texture is not None else None
            dst.vtx_offset, dst.idx_offset, dst.elem_count = int(c.vtx_offset), int(c.idx_offset), int(c.elem_count)
        dd = abi.UIDrawData()
        dd.display_pos[:] = draw.display_pos
        dd.display_size[:] = draw.display_size
        dd.framebuffer_scale[:] = draw.framebuffer_scale
        dd.d_vertices, dd.vertex_count = d_v.data_ptr(), len(draw.vertices)
        dd.d_indices, dd.index_count = d_i.data_ptr(), len(draw.indices)
        dd.commands, dd.command_count = commands, n
        return dd, (d_v, d_i, commands)

    def record(self, target, area, load_op, draw, handles, clear=BLACK, stream=None):
        dd, keep = self.draw_data(draw, handles)
        im = target.abi()
        rc = lib().szg_ui_layer_record_draw(self.h, stream, C.byref(im), abi.Rect(*area), load_op, (C.c_float * 4)(*clear), C.byref(dd))
        # the host command array may be overwritten as soon as the call returns
        C.memset(keep[2], 0xEE, C.sizeof(keep[2]))
        self.keep.append(keep)
        return rc


def run_case(layer, target, area, load_op, draw, textures, clear=BLACK):
    """Record `draw` on the GPU and return (bytes of the whole buffer, what the model expects there)."""
    handles = {k: layer.add_texture(t, pitch_pad=i % 3) for i, (k, t) in enumerate(textures.items())}
    rc = layer.record(target, area, load_op, draw, handles, clear)
    assert rc == abi.SZG_OK, lib().szg_last_error()
    got = target.read()
    for h in handles.values():
        assert layer.remove_texture(h) == abi.SZG_OK
    layer.keep.clear()
    want = target.expect(um.render(target.image0, area, load_op, clear, draw, textures))
    return got, want
