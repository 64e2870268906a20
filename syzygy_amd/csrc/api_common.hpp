// api_common.hpp — what the api_*.cpp units (the extern "C" boundary of include/szg/abi.h, one unit per pipeline) and
// szg_comm.cpp share on the host: error reporting, the argument checks (the predicates image_layout_ok, extents_ok,
// rect_inside, images_overlap; check_image for a pipeline's images, check_pass_image for the image of a pass without one),
// the device guard, the owner of device allocations, the staging ring, and the deferred pipeline's object, which
// api_deferred.cpp and api_raster.cpp both work on.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <type_traits>
#include <vector>

#include "szg/abi.h"
#include "szg/anisotropy.h"
#include "szg/mipmaps.h"
#include "szg_internal.hpp"
#include "szg_launch.hpp"

namespace szg
{
// Both set the calling thread's szg_last_error() text (one buffer per thread, api_core.cpp) and return the code.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int fail_hip(hipError_t e, const char* what);
// A HIP call that must succeed: on failure `cleanup` runs, then the error is reported as `what` and returned. A create
// function passes the destroy of its half-built object (whose buffers free themselves), so that a failed create leaves
// nothing behind and *out NULL.
#define SZG_HIP_OR(expr, cleanup, what)                                                                                        \
    do                                                                                                                         \
    {                                                                                                                          \
        hipError_t const _e = (expr);                                                                                          \
        if (_e != hipSuccess)                                                                                                  \
        {                                                                                                                      \
            cleanup;                                                                                                           \
            return szg::fail_hip(_e, what);                                                                                    \
        }                                                                                                                      \
    } while (0)
#define SZG_HIP(expr) SZG_HIP_OR(expr, (void)0, #expr)
// A step that has reported its own error: pass its code on.
#define SZG_TRY_RC(expr)                                                                                                       \
    do                                                                                                                         \
    {                                                                                                                          \
        int const _rc = (expr);                                                                                                \
        if (_rc != SZG_OK)                                                                                                     \
        {                                                                                                                      \
            return _rc;                                                                                                        \
        }                                                                                                                      \
    } while (0)

unsigned texel_bytes(unsigned fmt);
szg_image make_image(void* data, unsigned w, unsigned h, unsigned fmt);
// The conditions every image argument is held to, each written once (api_core.cpp). `data` and `pitch_bytes` are multiples
// of `bytes`:
bool rows_aligned(const void* data, unsigned pitch_bytes, unsigned bytes);
// natural layout: rows of `width` texels of `texel` bytes fit in the pitch, and pitch and data are multiples of `texel`
bool layout_ok(const void* data, unsigned width, unsigned pitch_bytes, unsigned texel);
bool image_layout_ok(const szg_image& im); // layout_ok of an image whose format is a known one
bool extents_ok(const szg_image& im, unsigned min); // both extents in [min, SZG_PRESENT_MAX_EXTENT]
bool rect_inside(const szg_rect& r, const szg_image& im);
bool images_overlap(const szg_image& a, const szg_image& b); // the bytes their texels occupy intersect
// An image must be present, of the expected format, at least w x h, with a
// pitch that covers its rows and keeps texels naturally aligned.
bool check_image(const szg_image& im, unsigned fmt, unsigned w, unsigned h, const char* name);
// An image argument `name` of the pass `me`: present with data, its format one of `formats` (`must` ends the refusal: "must
// be RGBA16_UNORM"). check_pass_image goes on: extents not above the cap, natural layout, `region` (optional) inside it.
bool check_image_format(const char* me, const char* name, const szg_image* im, std::initializer_list<unsigned> formats, const char* must);
bool check_image_layout(const char* me, const char* name, const szg_image& im);
bool check_pass_image(const char* me, const char* name, const szg_image* im, std::initializer_list<unsigned> formats, const char* must,
                      const szg_rect* region);
bool check_gbuffer(const szg_gbuffer* g, unsigned w, unsigned h);
bool check_scene(const szg_scene_texture* s, unsigned w, unsigned h, bool needDepth);
// VkRect2D offset: the reference dispatches every pass over the extent only and pushes gbufferOffset = 0
// (deferred.cpp:764, :778-787; skyview.cpp:658-665), i.e. it renders into the top-left sub-rectangle whatever the offset
// says. A caller passing a non-zero offset expects something this path (like the reference's) does not do: refuse it.
bool check_rect(const szg_rect& r, const char* what);
// Resolve the tile: returns false (with error) if inconsistent.
bool resolve_tile(const szg_rowtile* tile, unsigned drawH, TileArgs& out);
int select_device(int device);

// A pipeline lives on the device it was created on; record_* may be called while another device is current
// (one process driving several GPUs): switch for the duration of the call and switch back.
struct DeviceGuard
{
    int previous = -1;
    bool switched = false;
    explicit DeviceGuard(int device)
    {
        if (hipGetDevice(&previous) == hipSuccess && previous != device)
        {
            switched = hipSetDevice(device) == hipSuccess;
        }
    }
    ~DeviceGuard()
    {
        if (switched)
        {
            (void)hipSetDevice(previous);
        }
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// Owner of one hipMalloc allocation: move-only, freed with the object that holds it (on the device current at that time:
// the destroy functions set it). Reads as the plain pointer the launch interface takes.
template <typename T> class DeviceBuffer
{
    T* ptr = nullptr;

  public:
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& o) noexcept : ptr(o.ptr) { o.ptr = nullptr; }
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept
    {
        if (this != &o)
        {
            reset();
            ptr = o.ptr;
            o.ptr = nullptr;
        }
        return *this;
    }
    ~DeviceBuffer() { reset(); }
    void reset()
    {
        if (ptr != nullptr)
        {
            (void)hipFree(ptr);
            ptr = nullptr;
        }
    }
    // `count` elements (bytes of a DeviceBuffer<void>), optionally zero-filled; what was held before is freed first.
    // The zeros are there when alloc returns: hipMemset runs on the null stream, and neither its documentation nor
    // hipMemsetAsync's promises that a fill of device memory has completed when the call returns. A record call on a
    // non-blocking stream does not wait for the null stream, so alloc does (create time only).
    hipError_t alloc(size_t count, bool zero = false)
    {
        reset();
        size_t const bytes = count * sizeof(std::conditional_t<std::is_void<T>::value, char, T>);
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&ptr), bytes);
        if (e == hipSuccess && zero)
        {
            e = hipMemset(ptr, 0, bytes);
            if (e == hipSuccess)
            {
                e = hipStreamSynchronize(nullptr);
            }
        }
        return e;
    }
    T* get() const { return ptr; }
    operator T*() const { return ptr; }
};

// Small ring of pinned staging buffers for host -> device parameter uploads
// (the reference's TStagedBuffer staging half, buffers.hpp:209-299). A slot is
// reused only after the copy that read it has completed.
struct StagingRing
{
    static constexpr int SLOTS = 8;
    void* host[SLOTS] = {};
    hipEvent_t done[SLOTS] = {};
    bool used[SLOTS] = {};
    size_t bytes = 0;
    int next = 0;

    int init(size_t n)
    {
        bytes = n;
        for (int i = 0; i < SLOTS; i++)
        {
            SZG_HIP(hipHostMalloc(&host[i], n, hipHostMallocDefault));
            SZG_HIP(hipEventCreateWithFlags(&done[i], hipEventDisableTiming));
        }
        return SZG_OK;
    }
    StagingRing() = default;
    StagingRing(const StagingRing&) = delete;
    StagingRing& operator=(const StagingRing&) = delete;
    ~StagingRing()
    {
        for (int i = 0; i < SLOTS; i++)
        {
            if (done[i] != nullptr)
            {
                (void)hipEventDestroy(done[i]);
            }
            if (host[i] != nullptr)
            {
                (void)hipHostFree(host[i]);
            }
        }
    }
    // Copy `n` bytes from `src` (host) to `dst` (device) on `stream`.
    int upload(hipStream_t stream, void* dst, const void* src, size_t n)
    {
        if (n == 0)
        {
            return SZG_OK;
        }
        if (n > bytes)
        {
            return fail(SZG_ERR_CAPACITY, "staging upload of %zu bytes exceeds %zu", n, bytes);
        }
        int const s = next;
        next = (next + 1) % SLOTS;
        if (used[s])
        {
            SZG_HIP(hipEventSynchronize(done[s]));
        }
        std::memcpy(host[s], src, n);
        SZG_HIP(hipMemcpyAsync(dst, host[s], n, hipMemcpyHostToDevice, stream));
        SZG_HIP(hipEventRecord(done[s], stream));
        used[s] = true;
        return SZG_OK;
    }
};
} // namespace szg

// DeferredShadingPipeline: created, configured and recorded by api_deferred.cpp; api_raster.cpp records its mesh passes.
struct szg_deferred
{
    int device = 0;
    szg_deferred_desc desc{};
    szg_deferred_configuration config{};
    szg_gbuffer gbuffer{};
    szg::DeviceBuffer<void> d_gbufferPlanes[5];
    std::vector<szg_image> shadowImages; // host table returned by szg_deferred_shadow_maps
    szg_shadowmaps shadowMaps{};
    szg::DeviceBuffer<void> d_ownedShadowMaps;
    szg::DeviceBuffer<szg_spot_light_packed> d_spots;
    szg::DeviceBuffer<szg::ShadowSlot> d_slots;
    szg::DeviceBuffer<szg::LightRec> d_lightRecs;
    // per 64 x 64 tile of the capacity extent and per 64 light records one word (k_light_tiles), sized at creation; what the
    // last lights pass with spot lights wrote is tilesX x tilesY tiles of `batches` words (all 0: none yet)
    szg::DeviceBuffer<unsigned long long> d_lightTileMasks;
    unsigned lightTilesX = 0, lightTilesY = 0, lightTileBatches = 0;
    szg::DeviceBuffer<szg::ShadowSlot> d_ownedSlots; // the maps the pipeline allocated itself (never changes after create)
    szg::DeviceBuffer<szg::ShadowGen> d_shadowGen;
    szg::DeviceBuffer<szg_fill_box> d_boxes;
    unsigned maxBoxes = 1024;
    unsigned maxDirectional = 16;
    szg::StagingRing staging;
    // compute rasteriser (szg/raster.h): buffers grow on demand and are kept
    szg::DeviceBuffer<szg::RasterDraw> d_rasterDraws;
    size_t rasterDrawCapacity = 0;
    // the owners of what `raster` views (api_raster.cpp ensure_raster_capacity), named as in szg::RasterBuffers
    struct RasterStorage
    {
        szg::DeviceBuffer<szg::PrimRec> prims;
        szg::DeviceBuffer<uint2> boxes, orderedBoxes, chunkBoxes, superBoxes;
        szg::DeviceBuffer<unsigned> keysA, keysB, valsA, valsB;
        szg::DeviceBuffer<void> sortTemp;
    } rasterStorage;
    szg::RasterBuffers raster;
    // szg/mipmaps.h: the table of szg_deferred_set_texture_mips, looked up by level-0 pointer at record time
    std::vector<szg_texture_mips> textureMips;
    float textureMaxLod = SZG_SAMPLER_MAX_LOD_NONE;
    // szg/anisotropy.h: szg_deferred_set_sampler_anisotropy; above 1 the draws with a chain go to k_raster_tile_aniso
    float textureMaxAnisotropy = SZG_SAMPLER_MAX_ANISOTROPY_REFERENCE;
};

namespace szg
{
// Every refusal of an image or light argument of szg_deferred_record_lights without recording anything (api_deferred.cpp),
// reported under `caller`; `needDepth` when the same call also records a G-buffer pass into the scene texture. `plan`
// (optional) receives what the checks resolved.
struct LightsPlan
{
    TileArgs tile{};
    unsigned nDir = 0; // directional lights behind the skipped atmospheric ones
    bool empty = false; // zero-extent draw rect: nothing to record
};
int validate_lights(const char* caller, szg_deferred_t* p, szg_rect draw_rect, const szg_rowtile* tile,
                    const szg_scene_texture* scene_texture, uint32_t atmospheric_directional_lights_count,
                    const szg_directional_light_packed* d_directional_lights, uint32_t directional_light_count,
                    const szg_spot_light_packed* h_spot_lights, uint32_t spot_light_count, const szg_camera_packed* d_cameras,
                    bool needDepth, LightsPlan* plan);
} // namespace szg
