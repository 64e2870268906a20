// api_ui_layer.cpp — the UI layer pass behind the C-ABI (include/szg/ui_layer.h): the ImGui Vulkan backend's objects (textures,
// the per-frame buffers) and UILayer::recordDraw's render pass (uilayer.cpp:513-572).

#include <algorithm>
#include <cmath>
#include <memory>
#include <new>

#include "api_common.hpp"

using namespace szg;

// ImGui_ImplVulkan_AddTexture's descriptor set: a description of the image and its sampler
struct szg_ui_texture
{
    szg_image image{};
    szg_ui_sampler sampler{};
    uint32_t swizzle[4] = {}; // szg_ui_texture_view (szg/texture_display.h); all IDENTITY from szg_ui_layer_add_texture
};

struct szg_ui_layer
{
    int device = 0;
    uint32_t triangleCapacity = 0, commandCapacity = 0;
    std::vector<std::unique_ptr<szg_ui_texture>> textures;
    std::vector<UICommand> hostCommands; // the resolved commands of the record call in progress
    DeviceBuffer<UICommand> commands;
    DeviceBuffer<UIPrim> prims;
    DeviceBuffer<uint2> boxes, chunkBoxes, superBoxes;
    StagingRing staging;
    UILayerBuffers b{};
};

namespace
{
// the output or a texture: present, of one of `formats`, extents in [min, cap], rows inside the pitch, texels naturally aligned
bool check_ui_image(const char* caller, const char* name, const szg_image* im, unsigned min, std::initializer_list<unsigned> formats,
                    const char* must)
{
    if (!check_image_format(caller, name, im, formats, must))
    {
        return false;
    }
    if (!extents_ok(*im, min))
    {
        fail(SZG_ERR_INVALID_ARGUMENT, "%s: %s image %ux%u, extents must lie in [%u, %u]", caller, name, im->width, im->height, min,
             SZG_PRESENT_MAX_EXTENT);
        return false;
    }
    return check_image_layout(caller, name, *im);
}

szg_ui_texture* find_texture(szg_ui_layer* layer, const szg_ui_texture* t)
{
    for (auto const& owned : layer->textures)
    {
        if (owned.get() == t)
        {
            return owned.get();
        }
    }
    return nullptr;
}

// (int)x of VIEWPORT: truncated, saturating outside int32
int trunc_saturated(float x)
{
    if (x >= 2147483648.0f)
    {
        return INT32_MAX;
    }
    if (x <= -2147483648.0f)
    {
        return INT32_MIN;
    }
    return (int)x;
}

// ImGui_ImplVulkan_AddTexture behind both registrations: `view` NULL is the identity mapping, `allowHalf` admits RGBA16_SFLOAT
int add_texture(const char* me, szg_ui_layer* layer, const szg_image* image, szg_ui_sampler sampler, const szg_ui_texture_view* view,
                bool allowHalf, szg_ui_texture_t** out)
{
    if (layer == nullptr || out == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "%s: NULL argument", me);
    }
    *out = nullptr;
    bool const imageOk = allowHalf ? check_ui_image(me, "texture", image, 1u, {SZG_FORMAT_RGBA8_UNORM, SZG_FORMAT_RGBA16_UNORM, SZG_FORMAT_RGBA16_SFLOAT},
                                                    "must be RGBA8_UNORM, RGBA16_UNORM or RGBA16_SFLOAT")
                                   : check_ui_image(me, "texture", image, 1u, {SZG_FORMAT_RGBA8_UNORM, SZG_FORMAT_RGBA16_UNORM},
                                                    "must be RGBA8_UNORM or RGBA16_UNORM");
    if (!imageOk)
    {
        return SZG_ERR_INVALID_ARGUMENT;
    }
    if (sampler.filter != SZG_FILTER_NEAREST && sampler.filter != SZG_FILTER_LINEAR)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "%s: unknown filter %u", me, sampler.filter);
    }
    if (sampler.address != SZG_UI_ADDRESS_REPEAT && sampler.address != SZG_UI_ADDRESS_CLAMP_TO_EDGE &&
        sampler.address != SZG_UI_ADDRESS_CLAMP_TO_BORDER)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "%s: unknown address mode %u", me, sampler.address);
    }
    for (int i = 0; view != nullptr && i < 4; i++)
    {
        if (view->swizzle[i] > SZG_SWIZZLE_A)
        {
            return fail(SZG_ERR_INVALID_ARGUMENT, "%s: swizzle[%d] = %u is no component swizzle", me, i, view->swizzle[i]);
        }
    }
    std::unique_ptr<szg_ui_texture> t(new (std::nothrow) szg_ui_texture());
    if (!t)
    {
        return fail(SZG_ERR_OUT_OF_MEMORY, "%s: host allocation failed", me);
    }
    t->image = *image;
    t->sampler = sampler;
    for (int i = 0; view != nullptr && i < 4; i++)
    {
        t->swizzle[i] = view->swizzle[i];
    }
    *out = t.get();
    layer->textures.push_back(std::move(t));
    return SZG_OK;
}
} // namespace

extern "C" {

int szg_ui_layer_create(szg_ui_layer_t** out, uint32_t triangle_capacity, uint32_t command_capacity, int device)
{
    if (out == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_ui_layer_create: NULL argument");
    }
    *out = nullptr;
    if (triangle_capacity == 0u || triangle_capacity > SZG_UI_MAX_TRIANGLE_CAPACITY)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_ui_layer_create: triangle capacity %u outside [1, %u]", triangle_capacity,
                    SZG_UI_MAX_TRIANGLE_CAPACITY);
    }
    if (command_capacity == 0u || command_capacity > SZG_UI_MAX_COMMAND_CAPACITY)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_ui_layer_create: command capacity %u outside [1, %u]", command_capacity,
                    SZG_UI_MAX_COMMAND_CAPACITY);
    }
    SZG_TRY_RC(select_device(device));
    szg_ui_layer* p = new (std::nothrow) szg_ui_layer();
    if (p == nullptr)
    {
        return fail(SZG_ERR_OUT_OF_MEMORY, "szg_ui_layer_create: host allocation failed");
    }
    p->device = device;
    p->triangleCapacity = triangle_capacity;
    p->commandCapacity = command_capacity;
    p->hostCommands.reserve(command_capacity);
    size_t const chunks = ((size_t)triangle_capacity + 63u) / 64u;
    size_t const supers = (chunks + 63u) / 64u;
#define SZG_TRY(expr) SZG_HIP_OR(expr, szg_ui_layer_destroy(p), "szg_ui_layer_create")
    SZG_TRY(p->commands.alloc(command_capacity));
    SZG_TRY(p->prims.alloc(triangle_capacity));
    SZG_TRY(p->boxes.alloc(chunks * 64u));
    SZG_TRY(p->chunkBoxes.alloc(chunks));
    SZG_TRY(p->superBoxes.alloc(supers));
#undef SZG_TRY
    int const rc = p->staging.init((size_t)command_capacity * sizeof(UICommand));
    if (rc != SZG_OK)
    {
        szg_ui_layer_destroy(p);
        return rc;
    }
    p->b.commands = p->commands;
    p->b.prims = p->prims;
    p->b.boxes = p->boxes;
    p->b.chunkBoxes = p->chunkBoxes;
    p->b.superBoxes = p->superBoxes;
    *out = p;
    return SZG_OK;
}

void szg_ui_layer_destroy(szg_ui_layer_t* layer)
{
    if (layer == nullptr)
    {
        return;
    }
    (void)hipSetDevice(layer->device);
    (void)hipDeviceSynchronize();
    delete layer;
}

int szg_ui_layer_add_texture(szg_ui_layer_t* layer, const szg_image* image, szg_ui_sampler sampler, szg_ui_texture_t** out)
{
    return add_texture("szg_ui_layer_add_texture", layer, image, sampler, nullptr, false, out);
}

// include/szg/texture_display.h: the same registration with an image view, and RGBA16_SFLOAT among the formats
int szg_ui_layer_add_texture_view(szg_ui_layer_t* layer, const szg_image* image, szg_ui_sampler sampler, const szg_ui_texture_view* view,
                                  szg_ui_texture_t** out)
{
    return add_texture("szg_ui_layer_add_texture_view", layer, image, sampler, view, true, out);
}

int szg_ui_layer_remove_texture(szg_ui_layer_t* layer, szg_ui_texture_t* texture)
{
    if (layer == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "szg_ui_layer_remove_texture: NULL argument");
    }
    for (size_t i = 0; i < layer->textures.size(); i++)
    {
        if (layer->textures[i].get() == texture)
        {
            layer->textures.erase(layer->textures.begin() + (ptrdiff_t)i);
            return SZG_OK;
        }
    }
    return fail(SZG_ERR_INVALID_ARGUMENT, "szg_ui_layer_remove_texture: the texture is not this layer's");
}

// uilayer.cpp:513-572 -> ImGui_ImplVulkan_RenderDrawData. Everything up to the upload runs on the host, before anything is
// launched or written.
int szg_ui_layer_record_draw(szg_ui_layer_t* layer, void* stream, const szg_image* output, szg_rect render_area, uint32_t load_op,
                             const float clear_color[4], const szg_ui_draw_data* draw_data)
{
    static const char* const me = "szg_ui_layer_record_draw";
    if (layer == nullptr || draw_data == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "%s: NULL argument", me);
    }
    if (!check_ui_image(me, "output", output, 0u, {SZG_FORMAT_RGBA16_UNORM}, "must be RGBA16_UNORM"))
    {
        return SZG_ERR_INVALID_ARGUMENT;
    }
    szg_rect const& ra = render_area;
    if (!rect_inside(ra, *output))
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "%s: render area (%d, %d) %ux%u leaves the %ux%u image", me, ra.x, ra.y, ra.width, ra.height,
                    output->width, output->height);
    }
    if (load_op != SZG_UI_LOAD_OP_CLEAR && load_op != SZG_UI_LOAD_OP_LOAD)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "%s: unknown load op %u", me, load_op);
    }
    bool const clear = load_op == SZG_UI_LOAD_OP_CLEAR;
    if (clear && clear_color == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "%s: NULL clear colour under SZG_UI_LOAD_OP_CLEAR", me);
    }
    szg_ui_draw_data const& dd = *draw_data;
    for (int i = 0; i < 2; i++)
    {
        if (!std::isfinite(dd.display_pos[i]) || !std::isfinite(dd.display_size[i]) || !std::isfinite(dd.framebuffer_scale[i]))
        {
            return fail(SZG_ERR_INVALID_ARGUMENT, "%s: non-finite display_pos, display_size or framebuffer_scale", me);
        }
    }
    if (dd.command_count > 0u && dd.commands == nullptr)
    {
        return fail(SZG_ERR_INVALID_ARGUMENT, "%s: NULL command array with %u commands", me, dd.command_count);
    }
    if (dd.command_count > layer->commandCapacity)
    {
        return fail(SZG_ERR_CAPACITY, "%s: %u commands, capacity %u", me, dd.command_count, layer->commandCapacity);
    }
    // VIEWPORT
    int const fbw = trunc_saturated(dd.display_size[0] * dd.framebuffer_scale[0]);
    int const fbh = trunc_saturated(dd.display_size[1] * dd.framebuffer_scale[1]);
    // what limits every pixel whatever the command: render area ∩ viewport (the area lies inside the image)
    int64_t const lim[4] = {ra.x, ra.y, std::min<int64_t>((int64_t)ra.x + ra.width, fbw), std::min<int64_t>((int64_t)ra.y + ra.height, fbh)};
    std::vector<UICommand>& cmds = layer->hostCommands;
    cmds.clear();
    uint64_t submitted = 0u; // what the capacity is checked against: every command's triangles
    uint64_t triangles = 0u; // those of the commands that can draw
    for (uint32_t i = 0; i < dd.command_count; i++)
    {
        szg_ui_draw_cmd const& in = dd.commands[i];
        if (in.elem_count == 0u)
        {
            continue;
        }
        if (dd.d_vertices == nullptr || dd.d_indices == nullptr)
        {
            return fail(SZG_ERR_INVALID_ARGUMENT, "%s: NULL vertex or index array while command %u draws", me, i);
        }
        if (in.texture == nullptr)
        {
            return fail(SZG_ERR_INVALID_ARGUMENT, "%s: command %u has %u elements and a NULL texture", me, i, in.elem_count);
        }
        szg_ui_texture const* tex = find_texture(layer, in.texture);
        if (tex == nullptr)
        {
            return fail(SZG_ERR_INVALID_ARGUMENT, "%s: the texture of command %u is not this layer's", me, i);
        }
        if (images_overlap(tex->image, *output))
        {
            return fail(SZG_ERR_INVALID_ARGUMENT, "%s: the texture of command %u overlaps the output image in memory", me, i);
        }
        // ASSEMBLY: the index range truncated to the array, then whole triangles
        uint32_t const available = in.idx_offset < dd.index_count ? dd.index_count - in.idx_offset : 0u;
        uint32_t const tris = std::min(in.elem_count, available) / 3u;
        submitted += tris;
        if (submitted > layer->triangleCapacity)
        {
            return fail(SZG_ERR_CAPACITY, "%s: more than %u triangles (at command %u)", me, layer->triangleCapacity, i);
        }
        if (tris == 0u || dd.vertex_count == 0u || fbw <= 0 || fbh <= 0)
        {
            continue; // nothing of it can draw
        }
        // SCISSOR
        float cmin[2], cmax[2];
        bool skip = false;
        int64_t box[4];
        for (int a = 0; a < 2; a++)
        {
            cmin[a] = (in.clip_rect[a] - dd.display_pos[a]) * dd.framebuffer_scale[a];
            cmax[a] = (in.clip_rect[a + 2] - dd.display_pos[a]) * dd.framebuffer_scale[a];
            float const fb = (float)(a == 0 ? fbw : fbh);
            if (cmin[a] < 0.0f)
            {
                cmin[a] = 0.0f;
            }
            if (cmax[a] > fb)
            {
                cmax[a] = fb;
            }
            if (!std::isfinite(cmin[a]) || !std::isfinite(cmax[a]) || cmax[a] <= cmin[a])
            {
                skip = true;
                break;
            }
            // 0 <= cmin < cmax <= fb <= 2^31: both conversions are in range
            int64_t const o = (int32_t)cmin[a];
            int64_t const n = (uint32_t)(cmax[a] - cmin[a]);
            box[a] = std::max(o, lim[a]);
            box[a + 2] = std::min(o + n, lim[a + 2]);
            if (box[a + 2] <= box[a])
            {
                skip = true;
                break;
            }
        }
        if (skip)
        {
            continue;
        }
        UICommand c{};
        c.texData = tex->image.data;
        c.texWidth = tex->image.width;
        c.texHeight = tex->image.height;
        c.texPitch = tex->image.pitch_bytes;
        c.texFormat = tex->image.format == SZG_FORMAT_RGBA16_UNORM    ? UI_TEX_RGBA16_UNORM
                      : tex->image.format == SZG_FORMAT_RGBA16_SFLOAT ? UI_TEX_RGBA16_SFLOAT
                                                                      : UI_TEX_RGBA8_UNORM;
        for (unsigned k = 0; k < 4u; k++)
        {
            c.texFormat |= tex->swizzle[k] << (16u + 3u * k);
        }
        c.filter = tex->sampler.filter;
        c.address = tex->sampler.address;
        for (int k = 0; k < 4; k++)
        {
            c.clip[k] = (int)box[k];
        }
        c.vtxOffset = in.vtx_offset;
        c.firstIndex = in.idx_offset;
        c.triCount = tris;
        c.firstTri = (unsigned)triangles;
        triangles += tris;
        cmds.push_back(c);
    }
    if (ra.width == 0u || ra.height == 0u)
    {
        return SZG_OK;
    }
    DeviceGuard const guard(layer->device);
    hipStream_t const s = static_cast<hipStream_t>(stream);
    SZG_TRY_RC(layer->staging.upload(s, layer->commands, cmds.data(), cmds.size() * sizeof(UICommand)));
    UIDrawParams params{};
    params.displayPos[0] = dd.display_pos[0];
    params.displayPos[1] = dd.display_pos[1];
    params.scale[0] = dd.framebuffer_scale[0];
    params.scale[1] = dd.framebuffer_scale[1];
    params.vertices = dd.d_vertices;
    params.indices = dd.d_indices;
    params.vertexCount = dd.vertex_count;
    params.commandCount = (unsigned)cmds.size();
    params.triCount = (unsigned)triangles;
    float const none[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    SZG_HIP(szg::launch_ui_layer(s, *output, ra, clear, clear ? clear_color : none, params, layer->b));
    return SZG_OK;
}

} // extern "C"
