// canvas.hpp -- the reference's host-side classes around the render entry points, headless, over the C ABI of
// libsvr_hip.so (include/svr_abi.h, include/svr_io.h).  Same class and method names, same call order:
//
//   VolumeReader       core/VolumeReader.{h,cpp}      Read(.mhd/.mha), CreateDeviceVolume(cudaVolume*), sizes
//   TransferFunction   gui/transferfunction.{h,cpp}   node lists -> 1024 x RGBA table + maxOpacity, .tf save / load
//   Lights             core/lights/lights.{h,cpp}     environment light (.hdr or constant), area-light list
//   Canvas             gui/canvas.{h,cpp}             owns the scene PODs; every setter re-uploads through setup_* and
//                                                     restarts the progressive render; paintGL() renders one frame
//
// What is gone is Qt/OpenGL: paintGL() renders into a device image owned by the Canvas (the reference maps a GL
// pixel buffer), mouse / keyboard handlers become Rotate / Translate / Zoom calls, and the 0-ms timer that drives
// progressive refinement is the caller's loop.  The image size is a constructor argument (the reference's WIDTH /
// HEIGHT macros, common.h:8-9).
#ifndef SUNVOLUMERENDER_CANVAS_HPP
#define SUNVOLUMERENDER_CANVAS_HPP

#include <cmath>
#include <string>
#include <utility>
#include <vector>

#include "host_api.hpp"
#include "../svr_io.h"

// ---------------------------------------------------------------------------------------------------
// core/VolumeReader.h
// ---------------------------------------------------------------------------------------------------
class VolumeReader {
public:
    VolumeReader() = default;
    ~VolumeReader() { ClearDevice(); }
    VolumeReader(const VolumeReader&) = delete;                // owns a device texture
    VolumeReader& operator=(const VolumeReader&) = delete;

    // VolumeReader.cpp:13-77: the file is parsed on the host; cast, range, rescale, histogram and gradient-magnitude
    // maximum run on the GPU, and the texture is built at the same time (the reference does that in
    // CreateDeviceVolume; the result is the same object)
    void Read(std::string filename, int layout = SVR_LAYOUT_AUTO)
    {
        ClearDevice();
        layoutUsed = layout;
        histogram.assign(65536, 0u);
        svr_volume_info info;
        if ((keepVoxels ? ReadKeeping(filename, layout, &info) : svr_load_mhd(filename.c_str(), layout, &loaded, &info, histogram.data(), (uint32_t)histogram.size())) != 0) {
            ClearDevice();
            histogram.clear();
            return;                                   // svr_last_error() tells why (fatal mode has already exited)
        }
        histogram.resize(info.hist_bins < histogram.size() ? info.hist_bins : histogram.size());
        dim[0] = info.dim[0]; dim[1] = info.dim[1]; dim[2] = info.dim[2];
        spacing = glm::vec3(info.spacing[0], info.spacing[1], info.spacing[2]);
        maxMagnitude = info.maxMagnitude;
        range[0] = info.range[0]; range[1] = info.range[1];
        have = true;
    }

    // VolumeReader.cpp:174-185
    void CreateDeviceVolume(cudaVolume* volume)
    {
        if (!have) return;
        volume->bbox = loaded.bbox;
        volume->spacing = loaded.spacing;
        volume->invSpacing = loaded.invSpacing;
        volume->tex = loaded.tex;
        volume->SetInvMaxMagnitude(1.f / maxMagnitude);
    }

    glm::vec3 GetVolumeSize() { return glm::vec3(dim[0] * spacing.x, dim[1] * spacing.y, dim[2] * spacing.z); }
    float GetBoundingSphereRadius() { return glm::length(GetVolumeSize()) * 0.5f; }
    float GetElementBoundingSphereRadius() const { return glm::length(spacing) * 0.5f; }
    bool IsLoaded() const { return have; }

    // extension: keep the plain [z][y][x] u16 volume on the device after Read (set before Read; off by default, and then nothing
    // changes): what the region calls of Canvas segment and mask (svr_region_*)
    void KeepVoxels(bool keep) { keepVoxels = keep; }
    const uint16_t* DeviceVoxels() const { return voxels; }     // null unless KeepVoxels(true) was set before Read

    // extension: change the grid of the kept voxels (KeepVoxels(true)) after Read and before CreateDeviceVolume (svr_volume_resample;
    // include/svr_abi.h, "crop and resample").  dim, spacing, the texture and the box change -- the result is drawn where it lay inside
    // the loaded volume's box (svr_resample_grid_place) -- while maxMagnitude, range and histogram stay those of the loaded file.
    // Crop: the inclusive voxel box (x, y, z), cut to the volume
    int Crop(const int32_t box_min[3], const int32_t box_max[3])
    {
        if (!have || !voxels) return -4;
        svr_resample_grid grid;
        if (int rc = svr_resample_grid_box(dim, box_min, box_max, &grid)) return rc;
        return Regrid(grid, SVR_RESAMPLE_NEAREST);
    }
    // Resample: to target_spacing (x, y, z; the units of the file's spacing) under SVR_RESAMPLE_NEAREST / _LINEAR / _AREA / _AUTO; the
    // spacing applied is that of svr_resample_grid_spacing
    int Resample(const double target_spacing[3], int mode = SVR_RESAMPLE_AUTO)
    {
        if (!have || !voxels) return -4;
        const double sp[3] = {loaded.spacing.x, loaded.spacing.y, loaded.spacing.z};
        svr_resample_grid grid;
        if (int rc = svr_resample_grid_spacing(dim, sp, nullptr, nullptr, target_spacing, &grid, nullptr)) return rc;
        return Regrid(grid, mode);
    }

    std::vector<uint32_t> histogram;
    int dim[3] = {0, 0, 0};
    double range[2] = {0, 0};
    float maxMagnitude = 0.f;

private:
    void ClearDevice()
    {
        if (loaded.tex) svr_destroy_texture(loaded.tex);
        if (voxels) svr_device_free(voxels);
        voxels = nullptr;
        loaded = svr_volume();
        have = false;
    }
    // the kept voxels on `grid`: a new device volume and texture replace the old ones; on failure everything stays as it was
    int Regrid(const svr_resample_grid& grid, int mode)
    {
        const int32_t n[3] = {(int32_t)grid.axis[0].count, (int32_t)grid.axis[1].count, (int32_t)grid.axis[2].count};
        svr_volume placed;
        int rc = svr_resample_grid_place(&loaded, dim, &grid, &placed);
        if (rc != 0) return rc;
        uint16_t* out = (uint16_t*)svr_device_malloc((size_t)n[0] * n[1] * n[2] * sizeof(uint16_t));
        if (!out) return -4;
        rc = svr_volume_resample(voxels, dim, 1, &grid, mode, out);
        if (rc == 0) {
            placed.tex = svr_create_volume_texture(out, n[0], n[1], n[2], 1, layoutUsed);
            if (!placed.tex) rc = svr_last_error_code() ? svr_last_error_code() : -4;
        }
        svr_device_synchronize();
        if (rc != 0) { svr_device_free(out); return rc; }
        svr_destroy_texture(loaded.tex);
        svr_device_free(voxels);
        voxels = out;
        loaded = placed;
        for (int a = 0; a < 3; ++a) dim[a] = n[a];
        spacing = glm::vec3(loaded.spacing.x, loaded.spacing.y, loaded.spacing.z);
        return 0;
    }
    // svr_load_mhd in its parts, so that the preprocessed u16 volume stays: header, elements, GPU preprocessing, texture from the device
    // buffer; the svr_volume fields as svr_load_mhd fills them (VolumeReader.cpp:174-185, cuda_bbox.h)
    int ReadKeeping(const std::string& filename, int layout, svr_volume_info* info)
    {
        svr_mhd_header h;
        int rc = svr_mhd_read_header(filename.c_str(), &h);
        if (rc != 0) return rc;
        const size_t n = (size_t)h.dim[0] * h.dim[1] * h.dim[2];
        std::vector<uint8_t> elems(n * (size_t)h.elem_size);
        rc = svr_mhd_read_elements(&h, elems.data(), elems.size());
        if (rc != 0) return rc;
        voxels = (uint16_t*)svr_device_malloc(n * sizeof(uint16_t));
        if (!voxels) return -4;
        rc = svr_volume_preprocess(elems.data(), h.elem_type, h.dim[0], h.dim[1], h.dim[2], h.spacing, 0, voxels, histogram.data(),
                                   (uint32_t)histogram.size(), info);
        if (rc != 0) return rc;
        loaded.tex = svr_create_volume_texture(voxels, h.dim[0], h.dim[1], h.dim[2], 1, layout);
        if (!loaded.tex) return svr_last_error_code() ? svr_last_error_code() : -4;
        const float sx = info->spacing[0], sy = info->spacing[1], sz = info->spacing[2];
        const float ex = (float)h.dim[0] * sx, ey = (float)h.dim[1] * sy, ez = (float)h.dim[2] * sz;
        const float mx = ex - ex * 0.5f, my = ey - ey * 0.5f, mz = ez - ez * 0.5f;
        loaded.bbox.vmin = svr_vec3{-mx, -my, -mz};
        loaded.bbox.vmax = svr_vec3{mx, my, mz};
        loaded.bbox.invSize = svr_vec3{1.f / (mx - -mx), 1.f / (my - -my), 1.f / (mz - -mz)};
        loaded.spacing = svr_vec3{sx, sy, sz};
        loaded.invSpacing = svr_vec3{1.f / sx, 1.f / sy, 1.f / sz};
        loaded.invMaxMagnitude = 1.f / info->maxMagnitude;
        return 0;
    }
    glm::vec3 spacing;
    svr_volume loaded = svr_volume();
    bool have = false;
    bool keepVoxels = false;
    int layoutUsed = SVR_LAYOUT_AUTO;                          // Read's layout: Crop and Resample build their texture the same way
    uint16_t* voxels = nullptr;                                // the preprocessed volume (device), with KeepVoxels
};

// ---------------------------------------------------------------------------------------------------
// gui/transferfunction.h (vtkPiecewiseFunction + vtkColorTransferFunction node lists included)
// ---------------------------------------------------------------------------------------------------
class TransferFunction {
public:
    static const int TABLE_SIZE = SVR_TF_TABLE_SIZE;

    TransferFunction() = default;
    ~TransferFunction() { if (compositeTex) svr_destroy_texture(compositeTex); }
    TransferFunction(const TransferFunction&) = delete;        // owns a device texture
    TransferFunction& operator=(const TransferFunction&) = delete;

    // vtkPiecewiseFunction::AddPoint / vtkColorTransferFunction::AddRGBPoint: sorted by x, same x replaces
    void AddPoint(double x, double y, double midpoint = 0.5, double sharpness = 0.0)
    {
        const double node[4] = {x, y, midpoint, sharpness};
        Insert(opacity, 4, node);
    }
    void AddRGBPoint(double x, double r, double g, double b, double midpoint = 0.5, double sharpness = 0.0)
    {
        const double node[6] = {x, r, g, b, midpoint, sharpness};
        Insert(color, 6, node);
    }
    void RemoveAllPoints() { opacity.clear(); color.clear(); }
    int GetOpacitySize() const { return (int)opacity.size() / 4; }
    int GetColorSize() const { return (int)color.size() / 6; }

    // constructor body + onOpacityTFChanged / onColorTFChanged (transferfunction.cpp:17-44, 128-175): rebuild the
    // composite table and maxOpacity, (re)upload the 1-D texture; returns the texture handle
    cudaTextureObject_t Update()
    {
        svr_tf_build_table(opacity.data(), GetOpacitySize(), color.data(), GetColorSize(), TABLE_SIZE, compositeTable, &maxOpacity);
        if (compositeTex) svr_update_tf_texture(compositeTex, compositeTable, TABLE_SIZE, 0);
        else compositeTex = svr_create_tf_texture(compositeTable, TABLE_SIZE, 0);
        return compositeTex;
    }
    cudaTextureObject_t GetCompositeTFTextureObject() const { return compositeTex; }
    float GetMaxOpacityValue() const { return maxOpacity; }

    // transferfunction.cpp:55-126, without the file dialogs
    bool SaveCurrentTFConfiguration(const std::string& filename) const
    {
        return svr_tf_save(filename.c_str(), opacity.data(), GetOpacitySize(), color.data(), GetColorSize()) == 0;
    }
    bool LoadExistingTFConfiguration(const std::string& filename)
    {
        int n = 0, m = 0;
        if (svr_tf_load(filename.c_str(), nullptr, &n, nullptr, &m) != 0) return false;      // counts only
        std::vector<double> o((size_t)n * 4), c((size_t)m * 6);
        if (svr_tf_load(filename.c_str(), o.data(), &n, c.data(), &m) != 0) return false;
        RemoveAllPoints();
        for (int i = 0; i < n; ++i) Insert(opacity, 4, &o[(size_t)i * 4]);
        for (int i = 0; i < m; ++i) Insert(color, 6, &c[(size_t)i * 6]);
        return true;
    }

    float compositeTable[SVR_TF_TABLE_SIZE * 4] = {0};

private:
    static void Insert(std::vector<double>& nodes, int stride, const double* node)
    {
        size_t i = 0, n = nodes.size() / stride;
        while (i < n && nodes[i * stride] < node[0]) ++i;
        if (i < n && nodes[i * stride] == node[0]) { for (int k = 0; k < stride; ++k) nodes[i * stride + k] = node[k]; return; }
        nodes.insert(nodes.begin() + (long)(i * stride), node, node + stride);
    }
    std::vector<double> opacity, color;
    cudaTextureObject_t compositeTex = 0;
    float maxOpacity = 0.f;
};

// ---------------------------------------------------------------------------------------------------
// core/lights/lights.h
// ---------------------------------------------------------------------------------------------------
class Lights {
public:
    Lights() { environmentLight.Set(glm::vec3(0.03f)); }                       // lights.cpp:11-14
    ~Lights() { if (envTex) svr_destroy_texture(envTex); }
    Lights(const Lights&) = delete;                            // owns a device texture
    Lights& operator=(const Lights&) = delete;

    void SetEnvironmentLight(std::string filename)                              // lights.cpp:31-75
    {
        cudaTextureObject_t old = envTex;
        svr_environment_light tmp = environmentLight;
        if (svr_load_env_map(filename.c_str(), &tmp) != 0) return;
        environmentLight.Set(tmp.tex);
        envTex = tmp.tex;
        if (old) svr_destroy_texture(old);
    }
    void SetEnvionmentLight(const glm::vec3& radiance) { environmentLight.Set(radiance); }    // sic, lights.cpp:77
    void SetEnvironmentLightIntensity(float intensity) { environmentLight.SetIntensity(intensity); }
    void SetEnvironmentLightOffset(const glm::vec2& offset) { environmentLight.SetOffset(offset); }
    void AddAreaLights(const cudaAreaLight& areaLight, const glm::vec3& tm)     // lights.cpp:92-103
    {
        if (areaLights.size() <= SVR_MAX_LIGHT_SOURCES) { areaLights.push_back(areaLight); transforms.push_back(tm); }
        else fprintf(stderr, "Exceed maximum number of light sources\n");
    }
    void RemoveLights(uint32_t idx)
    {
        if (!areaLights.empty()) { areaLights.erase(areaLights.begin() + idx); transforms.erase(transforms.begin() + idx); }
    }

    cudaEnvironmentLight environmentLight;
    std::vector<cudaAreaLight> areaLights;
    std::vector<glm::vec3> transforms;

private:
    cudaTextureObject_t envTex = 0;
};

// ---------------------------------------------------------------------------------------------------
// gui/canvas.h
// ---------------------------------------------------------------------------------------------------
enum RenderMode { RENDER_MODE_PATHTRACER, RENDER_MODE_RAYCASTING, RENDER_MODE_PROJECTION /* extension: svr_render_projection with the SetProjection parameters */,
                  RENDER_MODE_SLICE /* extension: svr_render_slice with the SetSlice parameters */ };

class Canvas {
public:
    Canvas(int width, int height) : WIDTH(width), HEIGHT(height)              // canvas.cpp:8-20
    {
        volumeReader = new VolumeReader();
        lights.SetEnvionmentLight(glm::vec3(1.f));
        lights.SetEnvironmentLightIntensity(0.5f);
        setup_env_lights(lights.environmentLight);
        renderParams.SetupHDRBuffer(WIDTH, HEIGHT);
        renderParams.traceDepth = 1;
        deviceVolume.SetGradientFactor(0.5f);
        img = (glm::u8vec4*)svr_device_malloc((size_t)WIDTH * HEIGHT * 4);
        view[0] = glm::vec3(1.f, 0.f, 0.f); view[1] = glm::vec3(0.f, 1.f, 0.f); view[2] = glm::vec3(0.f, 0.f, 1.f);
    }
    ~Canvas()
    {
        svr_device_synchronize();
        ClearRegion();
        renderParams.Clear();
        if (img) svr_device_free(img);
        delete volumeReader;
    }
    Canvas(const Canvas&) = delete;
    Canvas& operator=(const Canvas&) = delete;

    void LoadVolume(std::string filename)                                       // canvas.cpp:27-41
    {
        ClearRegion();
        volumeReader->Read(filename);
        if (!volumeReader->IsLoaded()) return;
        volumeReader->CreateDeviceVolume(&deviceVolume);
        deviceVolume.SetClipPlane(glm::vec2(-1.f, 1.f), glm::vec2(-1.f, 1.f), glm::vec2(-1.f, 1.f));
        deviceVolume.SetDensityScale(1.f);
        setup_volume(deviceVolume);
        ZoomToExtent();
        view[0] = glm::vec3(1.f, 0.f, 0.f); view[1] = glm::vec3(0.f, 1.f, 0.f); view[2] = glm::vec3(0.f, 0.f, 1.f);
        cameraTranslate = glm::vec2(0.f, 0.f);
        UpdateCamera();
        ready = true;
        ReStartRender();
    }

    // extension: VolumeReader::Crop / Resample on the loaded volume (KeepVoxels(true) before LoadVolume); the Canvas then draws and
    // segments the new grid.  A region, a filtered copy and a shown region are dropped: they belonged to the old grid
    int CropVolume(const int32_t box_min[3], const int32_t box_max[3]) { return ready ? AdoptVolume(volumeReader->Crop(box_min, box_max)) : -4; }
    int ResampleVolume(const double target_spacing[3], int mode = SVR_RESAMPLE_AUTO) { return ready ? AdoptVolume(volumeReader->Resample(target_spacing, mode)) : -4; }

    void ReStartRender() { renderParams.frameNo = 0; }                          // canvas.h:43-47

    void SetTransferFunction(const cudaTextureObject_t& tex, float maxOpacity)  // canvas.h:49-54
    {
        transferFunction.Set(tex, maxOpacity);
        setup_transferfunction(transferFunction);
        ReStartRender();
    }
    void SetDensityScale(double s) { deviceVolume.SetDensityScale((float)s); setup_volume(deviceVolume); ReStartRender(); }
    void SetGradientFactor(double g) { deviceVolume.SetGradientFactor((float)g); setup_volume(deviceVolume); ReStartRender(); }
    void SetScatterTimes(double val) { renderParams.traceDepth = (uint32_t)val; ReStartRender(); }
    void SetRenderMode(RenderMode mode) { renderMode = mode; ReStartRender(); }
    // extension: what RENDER_MODE_PROJECTION draws (maximum / mean intensity projection, isosurface; include/svr_abi.h)
    void SetProjection(const svr_projection_params& p) { projection = p; ReStartRender(); }
    // extension: what RENDER_MODE_SLICE draws (a plane or slab through the volume; include/svr_abi.h)
    void SetSlice(const svr_slice_params& p) { slice = p; ReStartRender(); }
    // ... the plane perpendicular to world axis 0 / 1 / 2 at `position` in [0, 1] across the clipped box, fitted to the canvas; the slab
    // (thickness, step, mode), the window and the flags stay as they are.  Returns svr_slice_params_axis's status
    int SetSlice(int axis, float position)
    {
        svr_slice_params p;
        const int rc = svr_slice_params_axis(&p, &deviceVolume, axis, position, (uint32_t)WIDTH, (uint32_t)HEIGHT);
        if (rc != 0) return rc;
        slice.center = p.center; slice.u = p.u; slice.v = p.v;
        ReStartRender();
        return 0;
    }
    const svr_slice_params& Slice() const { return slice; }

    // lights, canvas.h:96-133
    void SetEnvLightBackground(const glm::vec3& color) { lights.SetEnvionmentLight(color); setup_env_lights(lights.environmentLight); ReStartRender(); }
    void SetEnvLightMap(std::string filename) { lights.SetEnvironmentLight(filename); setup_env_lights(lights.environmentLight); ReStartRender(); }
    void SetEnvLightOffset(const glm::vec2& offset) { lights.SetEnvironmentLightOffset(offset); setup_env_lights(lights.environmentLight); ReStartRender(); }
    void SetEnvLightIntensity(float intensity) { lights.SetEnvironmentLightIntensity(intensity); setup_env_lights(lights.environmentLight); ReStartRender(); }
    void SetAreaLights() { setup_area_lights(lights.areaLights.data(), (uint32_t)lights.areaLights.size()); ReStartRender(); }

    // camera, canvas.h:136-162
    void SetFOV(float f) { fov = f; UpdateCamera(); ReStartRender(); }
    void SetApeture(float a) { apeture = a; UpdateCamera(); ReStartRender(); }
    void SetFocalLength(float f) { focalLength = f; UpdateCamera(); ReStartRender(); }
    void SetExposure(float e) { exposure = e; UpdateCamera(); ReStartRender(); }

    // extension: edge-aware denoised image while a restarted render has at most `frames` samples per pixel (SVR_OPT_DENOISE_PREVIEW;
    // 0 = off).  Changes only the RGBA8 image, never the accumulator
    void SetDenoisePreview(int frames) { svr_set_option(SVR_OPT_DENOISE_PREVIEW, frames); }
    // extension: follow the render and estimate its remaining noise (SVR_OPT_NOISE_ESTIMATE); the latest estimate (frames == 0: none yet)
    void SetNoiseEstimate(bool on) { svr_set_option(SVR_OPT_NOISE_ESTIMATE, on ? 1 : 0); }
    // (the library keeps one estimate per process, of the render it last followed: one with another tile grid is another canvas's)
    svr_noise_estimate GetNoiseEstimate() const
    {
        svr_noise_estimate e = {};
        if (svr_get_noise_estimate(&e, nullptr) != 0 || e.tiles_x != (WIDTH + 15u) / 16u || e.tiles_y != (HEIGHT + 15u) / 16u) e = svr_noise_estimate{};
        return e;
    }

    // clip planes, canvas.h:165-184
    void SetXClipPlane(double mn, double mx) { deviceVolume.SetXClipPlane(glm::vec2(float(mn), float(mx))); setup_volume(deviceVolume); ReStartRender(); }
    void SetYClipPlane(double mn, double mx) { deviceVolume.SetYClipPlane(glm::vec2(float(mn), float(mx))); setup_volume(deviceVolume); ReStartRender(); }
    void SetZClipPlane(double mn, double mx) { deviceVolume.SetZClipPlane(glm::vec2(float(mn), float(mx))); setup_volume(deviceVolume); ReStartRender(); }

    // what the mouse / wheel / arrow-key handlers do to the view (canvas.cpp:119-226): rotate the view basis about
    // an axis given in view space, pan, dolly
    void Rotate(float angleDegrees, const glm::vec3& axis)
    {
        const float a = angleDegrees * 3.14159265358979323846f / 180.f, c = std::cos(a), s = std::sin(a);
        const glm::vec3 k = glm::normalize(axis);
        const glm::vec3 world = view[0] * k.x + view[1] * k.y + view[2] * k.z;
        for (int i = 0; i < 3; ++i)                                             // Rodrigues
            view[i] = view[i] * c + glm::cross(world, view[i]) * s + world * (glm::dot(world, view[i]) * (1.f - c));
        UpdateCamera();
        ReStartRender();
    }
    void Translate(const glm::vec2& delta) { cameraTranslate = glm::vec2(cameraTranslate.x + delta.x, cameraTranslate.y + delta.y); UpdateCamera(); ReStartRender(); }
    void Zoom(float delta) { eyeDist += delta; UpdateCamera(); ReStartRender(); }

    // paintGL's render branch, canvas.cpp:70-116
    void paintGL()
    {
        if (!ready) return;
        if (renderMode == RENDER_MODE_RAYCASTING)
            render_raycasting(img, deviceVolume, transferFunction, camera, volumeReader->GetElementBoundingSphereRadius());
        else if (renderMode == RENDER_MODE_PROJECTION)
            svr_render_projection(img, &deviceVolume, &transferFunction, &camera, volumeReader->GetElementBoundingSphereRadius(), &projection);
        else if (renderMode == RENDER_MODE_SLICE)
            svr_render_slice(img, &deviceVolume, &transferFunction, (uint32_t)WIDTH, (uint32_t)HEIGHT, &slice);
        else {
            render_pathtracer(img, renderParams);
            if (renderParams.frameNo == 0 && dumpFirstFrame) SaveImage("0.tga");   // canvas.cpp:97-104
        }
        svr_device_synchronize();
        renderParams.frameNo++;
    }

    // extension: n progressive frames in one launch group
    void paintFrames(uint32_t n)
    {
        if (!ready || renderMode != RENDER_MODE_PATHTRACER) return;
        svr_render_pathtracer_frames(img, &renderParams, n);
        renderParams.frameNo += n;
    }

    // extension: render until the predicted RMSE of the tone-mapped image is <= targetRmse (and every 16 x 16 tile's <= targetTileRmse; 0 =
    // unchecked) or maxFrames frames were traced (svr_render_pathtracer_until); frameNo advances by the frames traced, which are returned
    uint32_t RenderUntil(float targetRmse, float targetTileRmse, uint32_t maxFrames)
    {
        if (!ready || renderMode != RENDER_MODE_PATHTRACER) return 0;
        uint32_t done = 0;
        svr_render_pathtracer_until(img, &renderParams, targetRmse, targetTileRmse, maxFrames, &done);
        return done;
    }

    // extension: adaptive sampling (svr_render_pathtracer_adaptive): render on, freezing each 16 x 16 tile once its predicted RMSE was <=
    // targetTileRmse at two consecutive estimates (and it holds >= minFrames frames), until no tile is active or after maxFrames frames.
    // frameNo advances to the most frames a tile holds; the frozen tiles hold fewer, so ReStartRender before painting on.  Returns the
    // call's status (0 = ok); *result (may be null) gets svr_adaptive_result
    int PaintAdaptive(float targetTileRmse, uint32_t minFrames, uint32_t maxFrames, svr_adaptive_result* result = nullptr)
    {
        if (!ready || renderMode != RENDER_MODE_PATHTRACER) return -4;
        svr_adaptive_result r = {};
        const int rc = svr_render_pathtracer_adaptive(img, &renderParams, targetTileRmse, minFrames, maxFrames, &r);
        if (result) *result = r;
        return rc;
    }

    // extension: where the ray of pixel (x, y) meets what the picture shows (svr_pick with the canvas's scene; include/svr_abi.h, "hit maps
    // and picks"): one record into *hit (host memory).  Synchronises.  Returns the call's status (0 = ok)
    int Pick(uint32_t x, uint32_t y, svr_hit* hit, const svr_hit_params& params = svr_hit_params{SVR_HIT_OPACITY, 0.5f, 0.5f})
    {
        if (!ready || !hit) return -4;
        void* d = svr_device_malloc(sizeof(svr_hit));
        if (!d) return -4;
        const uint32_t xy[2] = {x, y};
        int rc = svr_pick(d, xy, 1u, &deviceVolume, &transferFunction, &camera, volumeReader->GetElementBoundingSphereRadius(), &params);
        if (rc == 0) rc = svr_memcpy_d2h(hit, d, sizeof(svr_hit));
        svr_device_free(d);
        return rc;
    }
    // ... and of every pixel: WIDTH x HEIGHT records, row-major, into `hits` (svr_render_hits).  Synchronises
    int HitMap(std::vector<svr_hit>& hits, const svr_hit_params& params = svr_hit_params{SVR_HIT_OPACITY, 0.5f, 0.5f})
    {
        if (!ready) return -4;
        hits.assign((size_t)WIDTH * HEIGHT, svr_hit{});
        const size_t bytes = hits.size() * sizeof(svr_hit);
        void* d = svr_device_malloc(bytes);
        if (!d) return -4;
        int rc = svr_memset_device(d, 0, bytes);          // (records outside a row shard or render window in force read as MISS)
        if (rc == 0) rc = svr_render_hits(d, &deviceVolume, &transferFunction, &camera, volumeReader->GetElementBoundingSphereRadius(), &params);
        if (rc == 0) rc = svr_memcpy_d2h(hits.data(), d, bytes);
        svr_device_free(d);
        return rc;
    }

    // extension: pick -> segment -> measure -> show (svr_region_*; include/svr_abi.h, "seeded region growing").  Needs the plain voxels:
    // volumeReader->KeepVoxels(true) before LoadVolume.
    // GrowRegion: the connected component (connectivity 6, 18 or 26) of the voxels with lo <= raw value <= hi around the voxel whose cell
    // holds hit.position (a FOUND record of Pick / HitMap); the Canvas keeps the mask, *stats (may be null) gets the statistics
    // (svr_region_measure turns them into volume, mean, deviation, centroid, surface area).  Returns the call's status (0 = ok)
    int GrowRegion(const svr_hit& hit, uint32_t lo, uint32_t hi, int connectivity, svr_region_stats* stats = nullptr)
    {
        const uint16_t* vox = SegVoxels();
        if (!ready || !vox || hit.status != SVR_HIT_STATUS_FOUND) return -4;
        const int* dim = volumeReader->dim;
        int32_t seed[3];
        int rc = svr_region_seed_from_world(&deviceVolume, dim[0], dim[1], dim[2], &hit.position, seed);
        if (rc != 0) return rc;
        if (!regionMask) regionMask = (uint32_t*)svr_device_malloc((size_t)svr_region_mask_words(dim[0], dim[1], dim[2]) * sizeof(uint32_t));
        if (!regionMask) return -4;
        svr_region_params p;
        svr_region_params_default(&p);
        p.lo = lo; p.hi = hi; p.connectivity = connectivity;
        svr_region_stats st = {};
        rc = svr_region_grow(vox, dim[0], dim[1], dim[2], 1, seed, 1u, &p, regionMask, &st);
        haveRegion = rc == 0;
        haveLabels = false;
        for (int a = 0; a < 3; ++a) regionSeed[a] = seed[a];     // DetachRegion starts from the same voxel, with the same connectivity
        regionConnectivity = connectivity;
        haveSeed = haveRegion;
        if (stats) *stats = st;
        return rc;
    }
    // Clean-up of the grown region (svr_region_morph / _fill_holes / _detach; include/svr_abi.h, "operations on region masks").  Each
    // replaces the Canvas's region mask by its result -- on failure the mask stays as it was -- and *stats (may be null) gets the
    // statistics of the new mask (svr_region_stats_of); ShowRegion then shows the cleaned region.
    // MorphRegion: SVR_MORPH_DILATE / _ERODE / _OPEN / _CLOSE by the unit element 6 / 18 / 26 applied `radius` times
    int MorphRegion(int op, int element, uint32_t radius, svr_region_stats* stats = nullptr)
    {
        if (!WorkMask()) return -4;
        const int* dim = volumeReader->dim;
        return ReplaceRegion(svr_region_morph(regionMask, dim[0], dim[1], dim[2], op, element, radius, regionWork), stats);
    }
    // FillRegionHoles: the region and every voxel outside it that cannot reach a face of the volume through the background
    int FillRegionHoles(int background_connectivity = 6, svr_region_stats* stats = nullptr)
    {
        if (!WorkMask()) return -4;
        const int* dim = volumeReader->dim;
        return ReplaceRegion(svr_region_fill_holes(regionMask, dim[0], dim[1], dim[2], background_connectivity, 0u, regionWork), stats);
    }
    // DetachRegion: what the region keeps around GrowRegion's seed voxel when connections thinner than the element (applied `radius`
    // times) are cut; a seed outside the region's opening leaves an empty region (stats->status == SVR_REGION_STATUS_EMPTY), return 0
    int DetachRegion(int element, uint32_t radius, svr_region_stats* stats = nullptr)
    {
        if (!WorkMask() || !haveSeed) return -4;
        const int* dim = volumeReader->dim;
        int32_t status = SVR_REGION_STATUS_OK;
        return ReplaceRegion(svr_region_detach(regionMask, dim[0], dim[1], dim[2], regionSeed, 1u, element, radius, regionConnectivity, 0u, regionWork, &status),
                             stats);
    }
    // Euclidean clean-up and measures of the region (svr_region_ball / _distance / _distance_max / _distance_volume; include/svr_abi.h,
    // "exact Euclidean distance maps").  Lengths are in the units of the loaded volume's spacing: svr_region_distance_weights turns the
    // spacing into integer weights and a unit, a length L is r2 = floor((L / unit)^2) and a map value d2 means sqrt(d2) * unit.
    // RegionDistanceUnits: those weights and that unit
    int RegionDistanceUnits(uint32_t weights[3], double* unit) const
    {
        const int* dim = volumeReader->dim;
        const double sp[3] = {deviceVolume.spacing.x, deviceVolume.spacing.y, deviceVolume.spacing.z};
        return svr_region_distance_weights(sp, dim[0], dim[1], dim[2], weights, unit);
    }
    // BallMorphRegion: SVR_MORPH_DILATE / _ERODE / _OPEN / _CLOSE by the ball of `radius` (>= 0, finite); replaces the region like MorphRegion
    int BallMorphRegion(int op, double radius, svr_region_stats* stats = nullptr)
    {
        if (!WorkMask()) return -4;
        if (!(radius >= 0.0) || !std::isfinite(radius)) return -3;
        uint32_t w[3];
        double unit = 0.0;
        if (int rc = RegionDistanceUnits(w, &unit)) return rc;
        const int* dim = volumeReader->dim;
        return ReplaceRegion(svr_region_ball(regionMask, dim[0], dim[1], dim[2], op, w, LengthToR2(radius, unit), regionWork), stats);
    }
    // RegionThickness: the largest ball inscribed in the region -- *radius = sqrt(max d2) * unit of the distance to the nearest voxel of the
    // volume outside the region, ijk = the first voxel (x, y, z) that attains it.  Returns SVR_REGION_STATUS_OK, or SVR_REGION_STATUS_EMPTY
    // (radius 0, ijk -1) for an empty region and for one that fills the volume; negative on an error.  The region stays as it is
    int RegionThickness(double* radius, int32_t ijk[3])
    {
        if (!ready || !SegVoxels() || !haveRegion || !radius || !ijk) return -4;
        uint32_t w[3];
        double unit = 0.0;
        if (int rc = RegionDistanceUnits(w, &unit)) return rc;
        const int* dim = volumeReader->dim;
        uint32_t* map = (uint32_t*)svr_device_malloc((size_t)dim[0] * dim[1] * dim[2] * sizeof(uint32_t));
        if (!map) return -4;
        uint32_t max_d2 = 0u, first = 0u;
        int32_t status = SVR_REGION_STATUS_EMPTY;
        int rc = svr_region_distance(regionMask, dim[0], dim[1], dim[2], w, SVR_DIST_TO_UNSET, map);
        if (rc == 0) rc = svr_region_distance_max(map, regionMask, dim[0], dim[1], dim[2], &max_d2, &first, &status);
        svr_device_free(map);
        if (rc != 0) return rc;
        *radius = 0.0;
        ijk[0] = ijk[1] = ijk[2] = -1;
        if (status == SVR_REGION_STATUS_EMPTY) return SVR_REGION_STATUS_EMPTY;
        *radius = std::sqrt((double)max_d2) * unit;
        ijk[0] = (int32_t)(first % (uint32_t)dim[0]);
        ijk[1] = (int32_t)(first / (uint32_t)dim[0] % (uint32_t)dim[1]);
        ijk[2] = (int32_t)(first / (uint32_t)dim[0] / (uint32_t)dim[1]);
        return SVR_REGION_STATUS_OK;
    }
    // ShowRegionDistance: every renderer now draws the distance map of the region -- to the region (SVR_DIST_TO_SET) or, inside it, to its
    // outside (SVR_DIST_TO_UNSET) -- as the volume min(65535, floor(sqrt(d2) * scale)), until ShowAll or the next volume
    int ShowRegionDistance(int target, uint32_t scale)
    {
        if (!ready || !SegVoxels() || !haveRegion) return -4;
        uint32_t w[3];
        double unit = 0.0;
        if (int rc = RegionDistanceUnits(w, &unit)) return rc;
        const int* dim = volumeReader->dim;
        const size_t n = (size_t)dim[0] * dim[1] * dim[2];
        uint32_t* map = (uint32_t*)svr_device_malloc(n * sizeof(uint32_t));
        uint16_t* shown = (uint16_t*)svr_device_malloc(n * sizeof(uint16_t));
        int rc = map && shown ? 0 : -4;
        if (rc == 0) rc = svr_region_distance(regionMask, dim[0], dim[1], dim[2], w, target, map);
        if (rc == 0) rc = svr_region_distance_volume(map, dim[0], dim[1], dim[2], scale, shown);
        if (rc == 0) rc = ShowVoxels(shown);
        if (map) svr_device_free(map);
        if (shown) svr_device_free(shown);
        return rc;
    }
    // The components of the region (svr_region_threshold / _label / _label_table / _select_by_size; include/svr_abi.h, "connected
    // components of region masks").
    // ThresholdRegion: the current region becomes every voxel with lo <= raw value <= hi -- the whole window, with no pick.  There is no
    // seed voxel then, so DetachRegion is refused (-4) until the next GrowRegion
    int ThresholdRegion(uint32_t lo, uint32_t hi, svr_region_stats* stats = nullptr)
    {
        const uint16_t* vox = SegVoxels();
        if (!ready || !vox) return -4;
        const int* dim = volumeReader->dim;
        if (!regionMask) regionMask = (uint32_t*)svr_device_malloc((size_t)svr_region_mask_words(dim[0], dim[1], dim[2]) * sizeof(uint32_t));
        if (!regionMask) return -4;
        const int rc = svr_region_threshold(vox, dim[0], dim[1], dim[2], 1, lo, hi, nullptr, nullptr, regionMask);
        haveRegion = rc == 0;
        haveSeed = false;
        haveLabels = false;
        if (rc != 0 || !stats) return rc;
        return svr_region_stats_of(vox, dim[0], dim[1], dim[2], 1, regionMask, stats);
    }
    // KeepLargestRegion: the k largest connected components (connectivity 6, 18 or 26) of the region, ties in size to the one that
    // starts first; RemoveSmallRegions: the components of at least min_voxels voxels.  An empty result is not an error
    // (stats->status == SVR_REGION_STATUS_EMPTY)
    int KeepLargestRegion(int k, int connectivity, svr_region_stats* stats = nullptr)
    {
        if (k < 1) return -3;
        return SelectRegionParts(0u, (uint32_t)k, connectivity, stats);
    }
    int RemoveSmallRegions(uint32_t min_voxels, int connectivity, svr_region_stats* stats = nullptr)
    {
        return SelectRegionParts(min_voxels, 0u, connectivity, stats);
    }
    // CountRegionParts: *count = the number of connected components of the region; the region stays as it is
    int CountRegionParts(int connectivity, uint32_t* count)
    {
        if (!ready || !SegVoxels() || !haveRegion || !count) return -4;
        const int* dim = volumeReader->dim;
        uint32_t* labels = (uint32_t*)svr_device_malloc((size_t)dim[0] * dim[1] * dim[2] * sizeof(uint32_t));
        if (!labels) return -4;
        const int rc = svr_region_label(regionMask, dim[0], dim[1], dim[2], connectivity, labels, count);
        svr_device_free(labels);
        return rc;
    }
    // Histograms of the segmented voxels (svr_volume_histogram, svr_histogram_*; include/svr_abi.h, "histograms of the u16 voxels"): of
    // the filtered copy when there is one, of the whole volume or, with insideRegion, of the voxels of the current region.
    // VolumeHistogram: counts = the 65536 >> shift bins of raw value >> shift
    int VolumeHistogram(uint32_t shift, std::vector<uint32_t>& counts, bool insideRegion = false)
    {
        const uint16_t* vox = SegVoxels();
        if (!ready || !vox || (insideRegion && !haveRegion)) return -4;
        svr_histogram_params p;
        svr_histogram_params_default(&p);
        p.shift = shift;
        uint32_t first = 0u, last = 0u;
        if (const int rc = svr_histogram_bin_range(&p, 0u, &first, &last)) return rc;            // (refuses a shift above 15)
        const uint32_t bins = svr_histogram_bins(&p);
        uint32_t* d = (uint32_t*)svr_device_malloc((size_t)bins * sizeof(uint32_t));
        if (!d) return -4;
        int rc = svr_volume_histogram(vox, volumeReader->dim, 1, insideRegion ? regionMask : nullptr, &p, d);
        counts.assign(bins, 0u);
        if (rc == 0) rc = svr_memcpy_d2h(counts.data(), d, (size_t)bins * sizeof(uint32_t));     // (waits for the stream)
        svr_device_free(d);
        return rc;
    }
    // OtsuRegion: the current region becomes class classIndex (1 .. classes, from dark to bright) of the exact Otsu thresholds of the
    // histogram at `shift` (classes = 2, or 3 with shift >= 8), through svr_histogram_bin_range and ThresholdRegion.  thresholds_raw
    // (classes - 1 values: the last raw value of each lower class) and window_raw (the class's lo, hi) are optional outputs
    int OtsuRegion(uint32_t classes, uint32_t classIndex, uint32_t shift, svr_region_stats* stats = nullptr, uint32_t* thresholds_raw = nullptr,
                   uint32_t* window_raw = nullptr)
    {
        if (classIndex < 1u || classIndex > classes) return -3;
        std::vector<uint32_t> counts;
        if (const int rc = VolumeHistogram(shift, counts)) return rc;
        uint32_t t[2] = {0u, 0u};
        if (const int rc = svr_histogram_otsu(counts.data(), (uint32_t)counts.size(), classes, t, nullptr)) return rc;
        svr_histogram_params p;
        svr_histogram_params_default(&p);
        p.shift = shift;
        const uint32_t firstBin = classIndex == 1u ? 0u : t[classIndex - 2u] + 1u;
        const uint32_t lastBin = classIndex == classes ? (uint32_t)counts.size() - 1u : t[classIndex - 1u];
        uint32_t lo = 0u, hi = 0u, skip = 0u;
        if (const int rc = svr_histogram_bin_range(&p, firstBin, &lo, &skip)) return rc;
        if (const int rc = svr_histogram_bin_range(&p, lastBin, &skip, &hi)) return rc;
        for (uint32_t k = 0; thresholds_raw && k + 1u < classes; ++k)
            if (const int rc = svr_histogram_bin_range(&p, t[k], &skip, &thresholds_raw[k])) return rc;
        if (window_raw) { window_raw[0] = lo; window_raw[1] = hi; }
        return ThresholdRegion(lo, hi, stats);
    }
    // AutoWindow: the quantiles numLo / den and numHi / den of the raw values (svr_histogram_quantile) as the grey window of slices and
    // projections, raw / 65535 x densityScale; a window of one value is opened by one raw step.  window_raw (optional): the two raw values
    int AutoWindow(uint32_t numLo, uint32_t numHi, uint32_t den, float* lo, float* hi, bool insideRegion = false, uint32_t* window_raw = nullptr)
    {
        if (!lo || !hi) return -4;
        if (numLo > numHi) return -3;
        std::vector<uint32_t> counts;
        if (const int rc = VolumeHistogram(0u, counts, insideRegion)) return rc;
        uint32_t a = 0u, b = 0u;
        if (const int rc = svr_histogram_quantile(counts.data(), (uint32_t)counts.size(), numLo, den, &a)) return rc;
        if (const int rc = svr_histogram_quantile(counts.data(), (uint32_t)counts.size(), numHi, den, &b)) return rc;
        if (window_raw) { window_raw[0] = a; window_raw[1] = b; }
        if (a == b) { if (b < 65535u) ++b; else --a; }
        *lo = (float)a / 65535.f * deviceVolume.densityScale;
        *hi = (float)b / 65535.f * deviceVolume.densityScale;
        return 0;
    }
    // RegionMedian: *raw = the median raw value of the region's voxels (the quantile 1 / 2); SVR_HISTOGRAM_STATUS_EMPTY for an empty region
    int RegionMedian(uint32_t* raw)
    {
        if (!raw) return -4;
        std::vector<uint32_t> counts;
        if (const int rc = VolumeHistogram(0u, counts, true)) return rc;
        return svr_histogram_quantile(counts.data(), (uint32_t)counts.size(), 1u, 2u, raw);
    }
    // Surface meshes (svr_mesh_region / _isosurface / _positions / _measure, svr_stl_write / svr_ply_write; include/svr_abi.h, "surface
    // meshes of region masks and isosurfaces").  ExtractRegionSurface: the closed surface of the current region after `relax` (0 ..
    // SVR_MESH_MAX_RELAX) constrained relaxation steps; ExtractIsoSurface: the surface {raw value >= level} of the segmented voxels.  The
    // canvas keeps the mesh on the host (SurfaceVertices: int32 x, y, z in 1/256 voxel on the padded grid; SurfaceTriangles: uint32
    // triples) until the next extraction.  An empty mesh is not an error (info->status == SVR_REGION_STATUS_EMPTY)
    int ExtractRegionSurface(uint32_t relax, svr_mesh_info* info = nullptr)
    {
        if (!ready || !haveRegion) return -4;
        const int* dim = volumeReader->dim;
        const svr_mesh_params p = {1u, relax};
        const uint32_t* mask = regionMask;
        return ExtractSurface([&](int32_t* v, uint64_t nv, uint32_t* t, uint64_t nt, svr_mesh_info* i) { return svr_mesh_region(mask, dim[0], dim[1], dim[2], &p, v, nv, t, nt, i); },
                              info);
    }
    int ExtractIsoSurface(uint32_t level, uint32_t relax, svr_mesh_info* info = nullptr)
    {
        const uint16_t* vox = SegVoxels();
        if (!ready || !vox) return -4;
        const int* dim = volumeReader->dim;
        const svr_mesh_params p = {level, relax};
        return ExtractSurface([&](int32_t* v, uint64_t nv, uint32_t* t, uint64_t nt, svr_mesh_info* i) { return svr_mesh_isosurface(vox, dim[0], dim[1], dim[2], 1, &p, v, nv, t, nt, i); },
                              info);
    }
    bool HasSurface() const { return haveSurface; }
    const std::vector<int32_t>& SurfaceVertices() const { return surfaceVertices; }
    const std::vector<uint32_t>& SurfaceTriangles() const { return surfaceTriangles; }
    // SaveSurface: the extracted surface in world coordinates (where the renderers draw the volume) as binary PLY for a name that ends in
    // ".ply", as binary STL otherwise
    int SaveSurface(const std::string& filename) const
    {
        if (!haveSurface) return -4;
        const uint64_t nv = surfaceVertices.size() / 3, nt = surfaceTriangles.size() / 3;
        std::vector<float> xyz(surfaceVertices.size());
        if (int rc = svr_mesh_positions(surfaceVertices.data(), nv, nullptr, &deviceVolume, xyz.data())) return rc;
        const bool ply = filename.size() >= 4 && (filename.compare(filename.size() - 4, 4, ".ply") == 0 || filename.compare(filename.size() - 4, 4, ".PLY") == 0);
        return (ply ? svr_ply_write : svr_stl_write)(filename.c_str(), xyz.data(), nv, surfaceTriangles.data(), nt);
    }
    // SurfaceMeasure: the volume the surface encloses (exact but for the last rounding) and its area, in the spacing's units
    int SurfaceMeasure(double* volume, double* area) const
    {
        if (!haveSurface || !volume || !area) return -4;
        const double sp[3] = {deviceVolume.spacing.x, deviceVolume.spacing.y, deviceVolume.spacing.z};
        const double scale[3] = {sp[0] / 256.0, sp[1] / 256.0, sp[2] / 256.0};
        const size_t vbytes = surfaceVertices.size() * sizeof(int32_t), tbytes = surfaceTriangles.size() * sizeof(uint32_t);
        int64_t vol6 = 0;
        *volume = *area = 0.0;
        if (!tbytes) return 0;
        char* buf = (char*)svr_device_malloc(vbytes + tbytes);
        if (!buf) return -4;
        int rc = svr_memcpy_h2d(buf, surfaceVertices.data(), vbytes);
        if (rc == 0) rc = svr_memcpy_h2d(buf + vbytes, surfaceTriangles.data(), tbytes);
        if (rc == 0) rc = svr_mesh_measure((const int32_t*)buf, surfaceVertices.size() / 3, (const uint32_t*)(buf + vbytes), surfaceTriangles.size() / 3, scale, &vol6, area);
        svr_device_free(buf);
        if (rc == 0) *volume = (double)vol6 / (6.0 * 256.0 * 256.0 * 256.0) * sp[0] * sp[1] * sp[2];
        return rc;
    }
    // Splitting and path lengths (svr_region_split / _zone_cut / _geodesic; include/svr_abi.h, "geodesic distances and influence zones").
    // SplitRegion: separates objects of the region that touch through necks thinner than a ball of neck_radius (> 0, finite, in the
    // spacing's units): the region is eroded by that ball, the cores are labelled under `connectivity`, every voxel goes to the core
    // nearest inside the region (moves weighted by their Euclidean length: svr_region_geodesic_weights) and a cut of one voxel is taken
    // between different parts.  *parts = the number of cores; the cut mask replaces the region like MorphRegion, so CountRegionParts,
    // KeepLargestRegion, RemoveSmallRegions and ShowRegion follow.  No core (*parts = 0) leaves an empty region, return 0
    int SplitRegion(double neck_radius, int connectivity, uint32_t* parts, svr_region_stats* stats = nullptr)
    {
        if (!WorkMask() || !parts) return -4;
        if (!(neck_radius > 0.0) || !std::isfinite(neck_radius)) return -3;
        uint32_t w[3], steps[7];
        double unit = 0.0, step_unit = 0.0;
        if (int rc = RegionDistanceUnits(w, &unit)) return rc;
        const int* dim = volumeReader->dim;
        const double sp[3] = {deviceVolume.spacing.x, deviceVolume.spacing.y, deviceVolume.spacing.z};
        if (int rc = svr_region_geodesic_weights(sp, connectivity, dim[0], dim[1], dim[2], steps, &step_unit)) return rc;
        uint32_t* zones = (uint32_t*)svr_device_malloc((size_t)dim[0] * dim[1] * dim[2] * sizeof(uint32_t));
        if (!zones) return -4;
        uint32_t count = 0u, unreached = 0u;
        int rc = svr_region_split(regionMask, dim[0], dim[1], dim[2], w, LengthToR2(neck_radius, unit), connectivity, steps, 0u, zones, &count, &unreached,
                                  nullptr);
        if (rc == 0) rc = svr_region_zone_cut(zones, dim[0], dim[1], dim[2], connectivity, regionWork);
        svr_device_free(zones);                                                 // (waits for the cut, which is asynchronous)
        if (rc == 0) *parts = count;
        return ReplaceRegion(rc, stats);
    }
    // RegionPathLength: *length = the length, in the spacing's units, of the shortest way inside the region between the voxels of two
    // picks (FOUND records of Pick / HitMap), by 26-moves weighted with their Euclidean lengths (about *length = d * unit; the chamfer
    // error is stated in include/svr_abi.h).  Returns SVR_REGION_STATUS_OK, or SVR_REGION_STATUS_EMPTY (length 0) when there is no way --
    // one of the voxels lies outside the region, or they lie in different parts of it; negative on an error.  The region stays as it is
    int RegionPathLength(const svr_hit& from, const svr_hit& to, double* length)
    {
        if (!ready || !SegVoxels() || !haveRegion || !length) return -4;
        if (from.status != SVR_HIT_STATUS_FOUND || to.status != SVR_HIT_STATUS_FOUND) return -4;
        const int* dim = volumeReader->dim;
        int32_t a[3], b[3];
        if (int rc = svr_region_seed_from_world(&deviceVolume, dim[0], dim[1], dim[2], &from.position, a)) return rc;
        if (int rc = svr_region_seed_from_world(&deviceVolume, dim[0], dim[1], dim[2], &to.position, b)) return rc;
        const double sp[3] = {deviceVolume.spacing.x, deviceVolume.spacing.y, deviceVolume.spacing.z};
        uint32_t steps[7];
        double unit = 0.0;
        if (int rc = svr_region_geodesic_weights(sp, 26, dim[0], dim[1], dim[2], steps, &unit)) return rc;
        const size_t n = (size_t)dim[0] * dim[1] * dim[2];
        uint32_t* labels = (uint32_t*)svr_device_malloc(n * sizeof(uint32_t));
        uint32_t* dist = (uint32_t*)svr_device_malloc(n * sizeof(uint32_t));
        int rc = labels && dist ? 0 : -4;
        if (rc == 0) rc = svr_region_seed_labels(a, 1u, dim[0], dim[1], dim[2], labels);
        if (rc == 0) rc = svr_region_geodesic(labels, regionMask, dim[0], dim[1], dim[2], steps, 0u, dist, nullptr, nullptr);
        uint32_t d = SVR_GEO_NONE;
        if (rc == 0) rc = svr_memcpy_d2h(&d, dist + (((size_t)b[2] * dim[1] + b[1]) * dim[0] + b[0]), sizeof d);
        if (labels) svr_device_free(labels);
        if (dist) svr_device_free(dist);
        if (rc != 0) return rc;
        *length = d == SVR_GEO_NONE ? 0.0 : (double)d * unit;
        return d == SVR_GEO_NONE ? SVR_REGION_STATUS_EMPTY : SVR_REGION_STATUS_OK;
    }
    // Grow from seeds (svr_region_growcut / _label_paint; include/svr_abi.h, "grow from seeds"): strokes of class 1, 2, ... on the picture,
    // then every voxel goes to the class whose strokes reach it over the path that crosses the least image contrast.
    // AddSeed: a stroke of class cls (1 .. SEED_MAX_CLASS) around the voxel of a pick (a FOUND record of Pick / HitMap): the ball of
    // brush_radius (>= 0, finite, in the spacing's units; 0 = the voxel alone) painted on the Canvas's marker map.  The first class
    // painted on a voxel stays.  The region, if there is one, stays as it is
    static constexpr uint32_t SEED_MAX_CLASS = 255u;
    int AddSeed(const svr_hit& hit, uint32_t cls, double brush_radius)
    {
        if (!ready || !SegVoxels() || hit.status != SVR_HIT_STATUS_FOUND) return -4;
        if (cls == 0u || cls > SEED_MAX_CLASS || !(brush_radius >= 0.0) || !std::isfinite(brush_radius)) return -3;
        const int* dim = volumeReader->dim;
        const int32_t dims[3] = {dim[0], dim[1], dim[2]};
        int32_t seed[3];
        if (int rc = svr_region_seed_from_world(&deviceVolume, dim[0], dim[1], dim[2], &hit.position, seed)) return rc;
        uint32_t w[3];
        double unit = 0.0;
        if (int rc = RegionDistanceUnits(w, &unit)) return rc;
        const size_t n = (size_t)dim[0] * dim[1] * dim[2], words = (size_t)svr_region_mask_words(dim[0], dim[1], dim[2]);
        if (!seedMarkers) {
            seedMarkers = (uint32_t*)svr_device_malloc(n * sizeof(uint32_t));
            if (!seedMarkers) return -4;
            seedMaxClass = 0u;
            if (int rc = svr_memset_device(seedMarkers, 0, n * sizeof(uint32_t))) { ClearSeeds(); return rc; }
        }
        uint32_t* masks = (uint32_t*)svr_device_malloc(2 * words * sizeof(uint32_t));      // the pick's voxel, and the ball around it
        if (!masks) return -4;
        const uint32_t bit = 1u << (seed[0] & 31);
        const size_t word = ((size_t)seed[2] * dim[1] + seed[1]) * ((size_t)(dim[0] + 31) / 32) + (size_t)(seed[0] >> 5);
        int rc = svr_memset_device(masks, 0, words * sizeof(uint32_t));
        if (rc == 0) rc = svr_memcpy_h2d(masks + word, &bit, sizeof bit);
        if (rc == 0) rc = svr_region_ball(masks, dim[0], dim[1], dim[2], SVR_MORPH_DILATE, w, LengthToR2(brush_radius, unit), masks + words);
        if (rc == 0) rc = svr_region_label_paint(seedMarkers, dims, masks + words, cls, 1);
        svr_device_free(masks);                                                           // (waits for the paint, which is asynchronous)
        if (rc == 0 && cls > seedMaxClass) seedMaxClass = cls;
        return rc;
    }
    void ClearSeeds()
    {
        if (seedMarkers) svr_device_free(seedMarkers);
        seedMarkers = nullptr;
        seedMaxClass = 0u;
    }
    // GrowFromSeeds: the classes of the strokes grown over the current region (inside_region) or over the whole volume.  params null =
    // svr_region_growcut_params_default(26).  *classes_found (may be null) = the classes that own at least one voxel.  The class map
    // becomes the region's labels -- OverlayRegionOnSlice, OverlayRegion and SaveRegionParts then show and save the classes -- and, grown
    // over the whole volume, the region becomes every voxel that got a class.  The strokes stay, for more of them and another run.
    // SVR_REGION_ERR_RANGE (costs reached the cap: raise contrast_shift) leaves the flagged result in place and is returned
    int GrowFromSeeds(const svr_growcut_params* params, bool inside_region, uint32_t* classes_found)
    {
        if (!ready || !SegVoxels() || !seedMarkers || (inside_region && !haveRegion)) return -4;
        const int* dim = volumeReader->dim;
        const int32_t dims[3] = {dim[0], dim[1], dim[2]};
        svr_growcut_params p;
        if (params) p = *params;
        else svr_region_growcut_params_default(&p, 26);
        const size_t n = (size_t)dim[0] * dim[1] * dim[2];
        if (!regionLabels) regionLabels = (uint32_t*)svr_device_malloc(n * sizeof(uint32_t));
        if (!regionMask) regionMask = (uint32_t*)svr_device_malloc((size_t)svr_region_mask_words(dim[0], dim[1], dim[2]) * sizeof(uint32_t));
        if (!regionLabels || !regionMask) return -4;
        haveLabels = false;
        const int grown = svr_region_growcut(SegVoxels(), dims, 1, seedMarkers, inside_region ? regionMask : nullptr, &p, nullptr, regionLabels, nullptr);
        if (grown != 0 && grown != SVR_REGION_ERR_RANGE) return grown;
        const uint32_t count = seedMaxClass;
        std::vector<uint8_t> keep(count + 1u, 1);
        std::vector<svr_region_component> table(count);
        char* d = (char*)svr_device_malloc(count * sizeof(svr_region_component) + keep.size());
        if (!d) return -4;
        int rc = svr_region_label_table(regionLabels, nullptr, dim[0], dim[1], dim[2], 1, count, (svr_region_component*)d);
        if (rc == 0) rc = svr_memcpy_d2h(table.data(), d, count * sizeof(svr_region_component));
        if (rc == 0 && !inside_region) {                                                  // the region: every voxel that got a class
            uint8_t* keep_device = (uint8_t*)(d + count * sizeof(svr_region_component));
            rc = svr_memcpy_h2d(keep_device, keep.data(), keep.size());
            if (rc == 0) rc = svr_region_select(regionLabels, dim[0], dim[1], dim[2], count, keep_device, regionMask);
            if (rc == 0) rc = svr_device_synchronize();
            haveRegion = rc == 0;
            haveSeed = false;
        }
        svr_device_free(d);
        if (rc != 0) return rc;
        haveLabels = true;
        labelClasses = count;
        labelCount = count;
        if (classes_found) {
            *classes_found = 0u;
            for (const svr_region_component& c : table) *classes_found += c.voxels ? 1u : 0u;
        }
        return grown;
    }
    // KeepSeedClass: the voxels of class cls of the last GrowFromSeeds become the region, like MorphRegion's result: ShowRegion,
    // ExtractRegionSurface and SaveRegion follow.  The class map goes with the region it belonged to
    int KeepSeedClass(uint32_t cls, svr_region_stats* stats = nullptr)
    {
        if (!WorkMask() || !haveLabels || labelClasses == 0u) return -4;
        if (cls == 0u || cls > labelClasses) return -3;
        const int* dim = volumeReader->dim;
        std::vector<uint8_t> keep(labelClasses + 1u, 0);
        keep[cls] = 1;
        uint8_t* keep_device = (uint8_t*)svr_device_malloc(keep.size());
        if (!keep_device) return -4;
        int rc = svr_memcpy_h2d(keep_device, keep.data(), keep.size());
        if (rc == 0) rc = svr_region_select(regionLabels, dim[0], dim[1], dim[2], labelClasses, keep_device, regionWork);
        svr_device_free(keep_device);                                                     // (waits for the select)
        if (rc == 0) labelClasses = 0u;
        return ReplaceRegion(rc, stats);
    }
    // extension: the region as an overlay on what is drawn (svr_overlay_slice, svr_render_hits + svr_hit_ids + svr_overlay_ids;
    // include/svr_abi.h, "overlays").  The region itself stays as it is.
    // LabelRegion: numbers the connected components of the region 1 .. *count (connectivity 6, 18 or 26) and keeps the labels next to the
    // mask: the overlays then give every part its own colour, until anything replaces the region
    int LabelRegion(int connectivity, uint32_t* count)
    {
        if (!ready || !SegVoxels() || !haveRegion || !count) return -4;
        const int* dim = volumeReader->dim;
        if (!regionLabels) regionLabels = (uint32_t*)svr_device_malloc((size_t)dim[0] * dim[1] * dim[2] * sizeof(uint32_t));
        if (!regionLabels) return -4;
        const int rc = svr_region_label(regionMask, dim[0], dim[1], dim[2], connectivity, regionLabels, count);
        haveLabels = rc == 0;
        labelClasses = 0u;                             // (parts, not the classes of GrowFromSeeds)
        labelCount = rc == 0 ? *count : 0u;
        return rc;
    }
    // OverlayRegionOnSlice: tints the slice image in img -- what RENDER_MODE_SLICE drew for `params` -- by the region: the labels when
    // they are current, else the mask.  style null = svr_overlay_style_default.  Synchronises
    int OverlayRegionOnSlice(const svr_slice_params& params, const svr_overlay_style* style = nullptr)
    {
        if (!ready || !haveRegion) return -4;
        const int* dim = volumeReader->dim;
        svr_overlay_style st;
        svr_overlay_style_default(&st);
        const svr_overlay_source src = RegionSource();
        const int rc = svr_overlay_slice(img, &deviceVolume, dim[0], dim[1], dim[2], (uint32_t)WIDTH, (uint32_t)HEIGHT, &params, 1u, 0.f, &src, style ? style : &st);
        return rc ? rc : svr_device_synchronize();
    }
    // OverlayRegion: tints the 3D picture in img (ray caster or projection) by the region: a pixel whose ray meets what the picture
    // shows -- the hit map of `params` -- in a voxel of the region gets that part's colour.  Synchronises
    int OverlayRegion(const svr_hit_params& params = svr_hit_params{SVR_HIT_OPACITY, 0.5f, 0.5f}, const svr_overlay_style* style = nullptr)
    {
        if (!ready || !haveRegion) return -4;
        const int* dim = volumeReader->dim;
        const size_t n = (size_t)WIDTH * HEIGHT;
        char* d = (char*)svr_device_malloc(n * (sizeof(svr_hit) + sizeof(uint32_t)));
        if (!d) return -4;
        uint32_t* ids = (uint32_t*)(d + n * sizeof(svr_hit));
        svr_overlay_style st;
        svr_overlay_style_default(&st);
        const svr_overlay_source src = RegionSource();
        int rc = svr_memset_device(d, 0, n * sizeof(svr_hit));          // (records outside a row shard or render window in force read as MISS)
        if (rc == 0) rc = svr_render_hits(d, &deviceVolume, &transferFunction, &camera, volumeReader->GetElementBoundingSphereRadius(), &params);
        if (rc == 0) rc = svr_hit_ids(ids, d, (uint32_t)WIDTH, (uint32_t)HEIGHT, &deviceVolume, dim[0], dim[1], dim[2], &src);
        if (rc == 0) rc = svr_overlay_ids(img, ids, (uint32_t)WIDTH, (uint32_t)HEIGHT, 1u, style ? style : &st);
        if (rc == 0) rc = svr_device_synchronize();
        svr_device_free(d);
        return rc;
    }
    const uint32_t* RegionLabels() const { return haveLabels ? regionLabels : nullptr; }   // device; one uint32 per voxel
    // ShowRegion: every renderer now draws the volume with the voxels outside (SVR_REGION_KEEP) or inside (SVR_REGION_REMOVE) the grown
    // region set to `fill`; ShowAll goes back to the loaded volume.  The Canvas owns the extra texture
    int ShowRegion(int mode, uint32_t fill)
    {
        const uint16_t* vox = SegVoxels();
        if (!ready || !vox || !haveRegion) return -4;
        const int* dim = volumeReader->dim;
        uint16_t* shown = (uint16_t*)svr_device_malloc((size_t)dim[0] * dim[1] * dim[2] * sizeof(uint16_t));
        if (!shown) return -4;
        int rc = svr_region_apply(vox, dim[0], dim[1], dim[2], 1, regionMask, mode, fill, shown);
        if (rc == 0) rc = ShowVoxels(shown);
        svr_device_free(shown);
        return rc;
    }
    // extension: filter the voxels before they are segmented (svr_volume_rank / _smooth; include/svr_abi.h, "exact volume filters").  The
    // result is a device copy that the Canvas owns; while one exists GrowRegion, ThresholdRegion, ShowRegion and the other region methods
    // read it in place of the loaded voxels.  Repeated calls stack: each filters the copy the last one left.  The loaded volume and
    // what is drawn do not change (ShowFiltered draws the copy).  Needs the plain voxels: volumeReader->KeepVoxels(true) before LoadVolume.
    // MedianVolume: the median over the unit element 6 / 18 / 26, `iterations` times
    int MedianVolume(int element, uint32_t iterations)
    {
        const int* dim = volumeReader->dim;
        const uint16_t* vox = SegVoxels();
        return ReplaceFiltered([&](uint16_t* out) { return svr_volume_rank(vox, dim[0], dim[1], dim[2], 1, SVR_FILTER_MEDIAN, element, iterations, out); });
    }
    // SmoothVolume: binomial smoothing of `sigma` in the units of the volume's spacing, the same length on every axis: the radii are
    // those of svr_volume_smooth_radii, so an axis with a coarse spacing gets a smaller radius (0 = it is left alone)
    int SmoothVolume(double sigma)
    {
        const int* dim = volumeReader->dim;
        const double sp[3] = {deviceVolume.spacing.x, deviceVolume.spacing.y, deviceVolume.spacing.z};
        uint32_t radii[3];
        if (int rc = svr_volume_smooth_radii(sp, sigma, radii, nullptr)) return rc;
        const uint16_t* vox = SegVoxels();
        return ReplaceFiltered([&](uint16_t* out) { return svr_volume_smooth(vox, dim[0], dim[1], dim[2], 1, radii, out); });
    }
    // UnfilterVolume: drops the copy; the region methods read the loaded voxels again.  A region made from the copy stays as it is
    void UnfilterVolume()
    {
        if (!filtered) return;
        svr_device_synchronize();
        svr_device_free(filtered);
        filtered = nullptr;
    }
    bool HasFiltered() const { return filtered != nullptr; }
    const uint16_t* FilteredVoxels() const { return filtered; }     // device, [nz][ny][nx]; null without a filter
    // ShowFiltered: every renderer now draws the filtered copy, until ShowAll or the next volume
    int ShowFiltered()
    {
        if (!ready || !filtered) return -4;
        return ShowVoxels(filtered);
    }
    void ShowAll()
    {
        if (!regionTex) return;
        volumeReader->CreateDeviceVolume(&deviceVolume);           // the loaded texture again (the other fields are the same)
        setup_volume(deviceVolume);
        svr_device_synchronize();
        svr_destroy_texture(regionTex);
        regionTex = 0;
        ReStartRender();
    }
    bool HasRegion() const { return haveRegion; }
    const uint32_t* RegionMask() const { return haveRegion ? regionMask : nullptr; }   // device; svr_region_mask_words words

    // extension: scissors (svr_stencil_polygon, svr_region_scissor_camera / _slice; include/svr_abi.h, "scissors").  polygon: the (x, y)
    // pairs of a closed line drawn on the picture, in pixels (the centre of pixel (px, py) is (px + 0.5, py + 0.5)), converted to 1/256
    // pixel by rounding to nearest; op: SVR_SCISSOR_ERASE_INSIDE / _ERASE_OUTSIDE / _FILL_INSIDE.  The region mask is changed in place;
    // *stats (may be null) gets the statistics of the new mask.  With no region yet, SVR_SCISSOR_FILL_INSIDE starts one from nothing.
    // ScissorRegion: through the canvas's camera, on the WIDTH x HEIGHT picture.  The projection takes the camera's frame u, v, w to be
    // orthonormal: a camera set up with an `up` that is not perpendicular to the view direction has shorter u and v, and cuts elsewhere
    int ScissorRegion(const std::vector<double>& polygon, int op, svr_region_stats* stats = nullptr)
    {
        return Scissor(nullptr, (uint32_t)WIDTH, (uint32_t)HEIGHT, polygon, op, 0.f, stats);
    }
    // ScissorRegionOnSlice: through slice 0 of `params` on a w x h slice picture, within the slab of `thickness` (world units) around the
    // plane; thickness <= 0 means the whole depth.  PaintRegionOnSlice adds the prism to the region
    int ScissorRegionOnSlice(const svr_slice_params& params, uint32_t w, uint32_t h, const std::vector<double>& polygon, int op, float thickness,
                             svr_region_stats* stats = nullptr)
    {
        return Scissor(&params, w, h, polygon, op, thickness, stats);
    }
    int PaintRegionOnSlice(const svr_slice_params& params, uint32_t w, uint32_t h, const std::vector<double>& polygon, float thickness,
                           svr_region_stats* stats = nullptr)
    {
        return Scissor(&params, w, h, polygon, SVR_SCISSOR_FILL_INSIDE, thickness, stats);
    }

    // extension: fill between slices (svr_region_slice_counts, svr_region_fill_between; include/svr_abi.h, "fill between slices").
    // axis: 0, 1, 2 = x, y, z.  RegionSliceCounts: the set voxels of every slice of the axis -- the slices that hold a drawing.
    // FillRegionBetweenSlices: every slice that holds a voxel of the region is a key, and the slices between consecutive keys are
    // filled by shape-based interpolation, in-plane distances in the volume's spacing (the weights of RegionDistanceUnits) -- so a
    // slice between two drawings is empty before the call, and to end a shape one calls svr_region_fill_between with explicit keys.  Replaces the region like MorphRegion; *info (may be null) tells the keys, gaps and filled slices
    int RegionSliceCounts(int axis, std::vector<uint64_t>& counts)
    {
        if (!ready || !SegVoxels() || !haveRegion) return -4;
        if (axis < 0 || axis > 2) return -3;
        const int* dim = volumeReader->dim;
        counts.assign((size_t)dim[axis], 0u);
        return svr_region_slice_counts(regionMask, dim[0], dim[1], dim[2], axis, counts.data());
    }
    int FillRegionBetweenSlices(int axis, svr_region_stats* stats = nullptr, svr_fill_between_info* info = nullptr)
    {
        if (!WorkMask()) return -4;
        svr_fill_between_params p;
        svr_fill_between_params_default(&p);
        p.axis = axis;
        double unit = 0.0;
        if (int rc = RegionDistanceUnits(p.weights, &unit)) return rc;
        const int* dim = volumeReader->dim;
        return ReplaceRegion(svr_region_fill_between(regionMask, dim[0], dim[1], dim[2], &p, regionWork, info), stats);
    }

    // extension: smoothing the region and its parts (svr_region_smooth / _label_smooth / _box_density; include/svr_abi.h, "smoothing
    // region masks and label maps").  Lengths are in the units of the volume's spacing, the same on every axis, so an axis with a coarse
    // spacing gets a smaller radius.
    // SmoothRegion: op SVR_SMOOTH_MAJORITY -- `size` is the edge of the window, the radii those of svr_region_smooth_radii -- or
    // SVR_SMOOTH_BINOMIAL -- `size` is the sigma, the radii those of svr_volume_smooth_radii -- applied `iterations` times.  Replaces the
    // region like MorphRegion
    int SmoothRegion(int op, double size, uint32_t iterations = 1, svr_region_stats* stats = nullptr)
    {
        if (!WorkMask()) return -4;
        if (op != SVR_SMOOTH_MAJORITY && op != SVR_SMOOTH_BINOMIAL) return -3;
        const int* dim = volumeReader->dim;
        const int32_t dims[3] = {dim[0], dim[1], dim[2]};
        const double sp[3] = {deviceVolume.spacing.x, deviceVolume.spacing.y, deviceVolume.spacing.z};
        uint32_t radii[3];
        if (int rc = op == SVR_SMOOTH_MAJORITY ? svr_region_smooth_radii(sp, size, radii, nullptr) : svr_volume_smooth_radii(sp, size, radii, nullptr)) return rc;
        int rc = svr_region_smooth(regionMask, dims, op, radii, iterations, regionWork, nullptr);
        if (rc == 0) rc = svr_device_synchronize();
        return ReplaceRegion(rc, stats);
    }
    // SmoothRegionParts: the mode filter over a window of edge `size` on the label map the canvas holds -- the parts of LabelRegion
    // (after SplitRegion too) or the classes of GrowFromSeeds, at most SVR_LABEL_SMOOTH_MAX_COUNT of them (-3 beyond) -- all parts at
    // once, so that they stay disjoint and leave no gaps.  The region becomes every voxel that still has a label; *changed (may be null)
    // = the voxels whose label changed
    int SmoothRegionParts(double size, uint32_t iterations = 1, uint64_t* changed = nullptr)
    {
        if (!ready || !SegVoxels() || !haveRegion || !haveLabels) return -4;
        if (labelCount == 0u || labelCount > SVR_LABEL_SMOOTH_MAX_COUNT) return -3;
        const int* dim = volumeReader->dim;
        const int32_t dims[3] = {dim[0], dim[1], dim[2]};
        const double sp[3] = {deviceVolume.spacing.x, deviceVolume.spacing.y, deviceVolume.spacing.z};
        uint32_t radii[3];
        if (int rc = svr_region_smooth_radii(sp, size, radii, nullptr)) return rc;
        const std::vector<uint8_t> keep(labelCount + 1u, 1);
        uint32_t* smoothed = (uint32_t*)svr_device_malloc((size_t)dim[0] * dim[1] * dim[2] * sizeof(uint32_t));
        uint8_t* keep_device = (uint8_t*)svr_device_malloc(keep.size());
        int rc = smoothed && keep_device ? 0 : -4;
        if (rc == 0) rc = svr_region_label_smooth(regionLabels, dims, labelCount, radii, iterations, smoothed, changed);
        if (rc == 0) rc = svr_memcpy_h2d(keep_device, keep.data(), keep.size());
        if (rc == 0) rc = svr_region_select(smoothed, dim[0], dim[1], dim[2], labelCount, keep_device, regionMask);
        if (rc == 0) rc = svr_device_synchronize();
        if (rc == 0) std::swap(regionLabels, smoothed);
        if (smoothed) svr_device_free(smoothed);
        if (keep_device) svr_device_free(keep_device);
        return rc;
    }
    // ShowRegionDensity: every renderer now draws the local volume fraction of the region -- the share of set voxels in the window of
    // edge `size` around every voxel, 65535 = all of them (BV/TV of a bone mask) -- until ShowAll or the next volume
    int ShowRegionDensity(double size)
    {
        if (!ready || !SegVoxels() || !haveRegion) return -4;
        const int* dim = volumeReader->dim;
        const int32_t dims[3] = {dim[0], dim[1], dim[2]};
        const double sp[3] = {deviceVolume.spacing.x, deviceVolume.spacing.y, deviceVolume.spacing.z};
        uint32_t radii[3];
        if (int rc = svr_region_smooth_radii(sp, size, radii, nullptr)) return rc;
        uint16_t* shown = (uint16_t*)svr_device_malloc((size_t)dim[0] * dim[1] * dim[2] * sizeof(uint16_t));
        if (!shown) return -4;
        int rc = svr_region_box_density(regionMask, dims, radii, shown);
        if (rc == 0) rc = ShowVoxels(shown);
        svr_device_free(shown);
        return rc;
    }

    // extension: how far the region is from another mask of the same dimensions (svr_region_compare / _compare_measure; include/svr_abi.h,
    // "comparing segmentations").  The region is A, the other mask B; distances are in the units of the loaded volume's spacing (mm), by
    // the weights and unit of RegionDistanceUnits.  tolerances (may be null) are ntol <= SVR_COMPARE_MAX_TOLERANCES lengths in those units
    // for the surface Dice.  comparison (may be null) receives the integers.  The region stays as it is
    int CompareRegion(const uint32_t* otherMaskDevice, svr_compare_measurement* out, svr_region_comparison* comparison = nullptr, int element = 6,
                      const double* tolerances = nullptr, uint32_t ntol = 0u)
    {
        if (!ready || !haveRegion || !otherMaskDevice || !out) return -4;
        if (ntol > SVR_COMPARE_MAX_TOLERANCES || (ntol && !tolerances)) return -3;
        svr_compare_params p;
        svr_compare_params_default(&p);
        double unit = 0.0;
        if (int rc = RegionDistanceUnits(p.weights, &unit)) return rc;
        p.element = element;
        p.ntol = ntol;
        for (uint32_t k = 0; k < ntol; ++k) {
            if (!(tolerances[k] >= 0.0) || !std::isfinite(tolerances[k])) return -3;
            p.tolerances2[k] = LengthToR2(tolerances[k], unit);
        }
        const int* dim = volumeReader->dim;
        svr_region_comparison c;
        if (int rc = svr_region_compare(regionMask, otherMaskDevice, dim[0], dim[1], dim[2], &p, &c)) return rc;
        if (comparison) *comparison = c;
        return svr_region_compare_measure(&c, unit, out);
    }
    // CompareRegionWithFile: the same against a mask MetaImage of one byte per voxel as SaveRegion writes it, non-zero = set; the file
    // must have the dimensions of the loaded volume (-3 otherwise)
    int CompareRegionWithFile(const std::string& filename, svr_compare_measurement* out, svr_region_comparison* comparison = nullptr, int element = 6,
                              const double* tolerances = nullptr, uint32_t ntol = 0u)
    {
        if (!ready || !haveRegion || !out) return -4;
        const int* dim = volumeReader->dim;
        svr_mhd_header h;
        int rc = svr_mhd_read_header(filename.c_str(), &h);
        if (rc != 0) return rc;
        if (h.elem_size != 1 || h.dim[0] != dim[0] || h.dim[1] != dim[1] || h.dim[2] != dim[2]) return -3;
        const size_t n = (size_t)dim[0] * dim[1] * dim[2];
        std::vector<uint8_t> bytes(n);
        rc = svr_mhd_read_elements(&h, bytes.data(), bytes.size());
        if (rc != 0) return rc;
        std::vector<uint16_t> set(n);
        for (size_t i = 0; i < n; ++i) set[i] = bytes[i] ? 1u : 0u;
        uint32_t* other = (uint32_t*)svr_device_malloc((size_t)svr_region_mask_words(dim[0], dim[1], dim[2]) * sizeof(uint32_t));
        if (!other) return -4;
        rc = svr_region_threshold(set.data(), dim[0], dim[1], dim[2], 0, 1u, 65535u, nullptr, nullptr, other);      // (a host source: synchronises)
        if (rc == 0) rc = CompareRegion(other, out, comparison, element, tolerances, ntol);
        svr_device_free(other);
        return rc;
    }
    // MatchRegionParts: which part of LabelRegion's label map (counts parts) is which part of another label map of the same dimensions
    // (otherLabelsDevice, labels 1 .. otherCount): bestOther[l - 1] = the part of the other map with the largest Jaccard index with part
    // l, 0 for none, bestMine (may be null) the other way round (svr_region_label_overlap, svr_overlap_match).  table (may be null)
    // receives the overlap table [count + 1][otherCount + 1]
    int MatchRegionParts(uint32_t count, const uint32_t* otherLabelsDevice, uint32_t otherCount, std::vector<uint32_t>* bestOther,
                         std::vector<uint32_t>* bestMine = nullptr, std::vector<uint32_t>* table = nullptr)
    {
        if (!ready || !haveRegion || !haveLabels || !otherLabelsDevice || !bestOther) return -4;
        if (count == 0u || otherCount == 0u) return -3;
        const int32_t dims[3] = {volumeReader->dim[0], volumeReader->dim[1], volumeReader->dim[2]};
        const size_t cells = ((size_t)count + 1u) * ((size_t)otherCount + 1u);
        if (cells > SVR_HISTOGRAM_MAX_CELLS) return -3;
        uint32_t* d = (uint32_t*)svr_device_malloc(cells * sizeof(uint32_t));
        if (!d) return -4;
        std::vector<uint32_t> t(cells);
        int rc = svr_region_label_overlap(regionLabels, count, otherLabelsDevice, otherCount, dims, d);
        if (rc == 0) rc = svr_memcpy_d2h(t.data(), d, cells * sizeof(uint32_t));
        svr_device_free(d);
        if (rc != 0) return rc;
        bestOther->assign(count, 0u);
        if (bestMine) bestMine->assign(otherCount, 0u);
        rc = svr_overlap_match(t.data(), count, otherCount, bestOther->data(), bestMine ? bestMine->data() : nullptr);
        if (table) table->swap(t);
        return rc;
    }

    // extension: what the region methods read and made, as MetaImage files (svr_mhd_write, include/svr_io.h; a name ending in .mha gives
    // one file, any other a header and a .raw).  ElementSpacing is the drawn volume's, Offset the world position of the centre of voxel
    // (0, 0, 0) in the Canvas's box.  The Canvas's own state and dimensions do not change.
    // SaveVolume: the voxels the region methods read (the filtered copy when there is one), u16
    int SaveVolume(const std::string& filename)
    {
        if (!ready || !SegVoxels()) return -4;
        const int* dim = volumeReader->dim;
        return SaveDeviceArray(filename, SegVoxels(), SVR_ELEM_U16, sizeof(uint16_t), dim, deviceVolume);
    }
    // SaveRegion: the region's mask as u8, 1 inside and 0 outside (svr_region_mask_expand); svr_region_threshold with the window 1 .. 65535
    // on the loaded file gives the mask back
    int SaveRegion(const std::string& filename)
    {
        if (!ready || !haveRegion) return -4;
        const int* dim = volumeReader->dim;
        return SaveMask(filename, regionMask, dim, deviceVolume);
    }
    // SaveRegionParts: LabelRegion's label map as u32
    int SaveRegionParts(const std::string& filename)
    {
        if (!ready || !haveRegion || !haveLabels) return -4;
        const int* dim = volumeReader->dim;
        return SaveDeviceArray(filename, regionLabels, SVR_ELEM_U32, sizeof(uint32_t), dim, deviceVolume);
    }
    // SaveRegionCrop: the region's bounding box grown by margin_voxels on every side and cut to the volume: the voxels and the mask,
    // cropped on the GPU (svr_volume_resample, svr_region_resample), with the Offset of where the box lies.  crop_dims (may be null) gets
    // the box's dimensions.  An empty region has no box: SVR_REGION_STATUS_EMPTY is returned and nothing is written
    int SaveRegionCrop(const std::string& volume_file, const std::string& mask_file, int margin_voxels, int32_t crop_dims[3] = nullptr)
    {
        if (!ready || !SegVoxels() || !haveRegion) return -4;
        if (margin_voxels < 0) return -3;
        const int* dim = volumeReader->dim;
        svr_region_stats st;
        int rc = svr_region_stats_of(SegVoxels(), dim[0], dim[1], dim[2], 1, regionMask, &st);
        if (rc != 0) return rc;
        if (st.status == SVR_REGION_STATUS_EMPTY) return SVR_REGION_STATUS_EMPTY;
        int32_t lo[3], hi[3];
        for (int a = 0; a < 3; ++a) {
            lo[a] = st.bbox_min[a] > margin_voxels ? st.bbox_min[a] - margin_voxels : 0;
            hi[a] = st.bbox_max[a] < dim[a] - margin_voxels ? st.bbox_max[a] + margin_voxels : dim[a] - 1;
        }
        svr_resample_grid grid;
        svr_volume placed;
        rc = svr_resample_grid_box(dim, lo, hi, &grid);
        if (rc == 0) rc = svr_resample_grid_place(&deviceVolume, dim, &grid, &placed);
        if (rc != 0) return rc;
        const int n[3] = {(int)grid.axis[0].count, (int)grid.axis[1].count, (int)grid.axis[2].count};
        const size_t voxels = (size_t)n[0] * n[1] * n[2];
        uint16_t* vol = (uint16_t*)svr_device_malloc(voxels * sizeof(uint16_t));
        uint32_t* mask = (uint32_t*)svr_device_malloc((size_t)svr_region_mask_words(n[0], n[1], n[2]) * sizeof(uint32_t));
        rc = vol && mask ? 0 : -4;
        if (rc == 0) rc = svr_volume_resample(SegVoxels(), dim, 1, &grid, SVR_RESAMPLE_NEAREST, vol);
        if (rc == 0) rc = svr_region_resample(regionMask, dim, &grid, mask);
        if (rc == 0) rc = SaveDeviceArray(volume_file, vol, SVR_ELEM_U16, sizeof(uint16_t), n, placed);
        if (rc == 0) rc = SaveMask(mask_file, mask, n, placed);
        svr_device_synchronize();
        if (vol) svr_device_free(vol);
        if (mask) svr_device_free(mask);
        if (rc == 0 && crop_dims) for (int a = 0; a < 3; ++a) crop_dims[a] = n[a];
        return rc;
    }

    bool SaveImage(const std::string& filename)
    {
        std::vector<uint8_t> host((size_t)WIDTH * HEIGHT * 4);
        if (svr_memcpy_d2h(host.data(), img, host.size()) != 0) return false;
        return svr_tga_write(filename.c_str(), WIDTH, HEIGHT, host.data()) == 0;
    }
    void ReadImage(std::vector<uint8_t>& host)
    {
        host.resize((size_t)WIDTH * HEIGHT * 4);
        svr_memcpy_d2h(host.data(), img, host.size());
    }

    uint32_t FrameNo() const { return renderParams.frameNo; }
    void* HdrBuffer() const { return renderParams.hdrBuffer; }               // the accumulator (device): what svr_assemble_frame sends
    const cudaCamera& Camera() const { return camera; }
    const cudaVolume& Volume() const { return deviceVolume; }
    const cudaTransferFunction& TransferFunctionPod() const { return transferFunction; }   // (TransferFunction is the editor class above)

    VolumeReader* volumeReader;
    Lights lights;
    bool dumpFirstFrame = false;                   // the reference always writes 0.tga; off by default here

    const int WIDTH, HEIGHT;

private:
    void ZoomToExtent()                                                         // canvas.cpp:191-197
    {
        glm::vec3 extent = volumeReader->GetVolumeSize();
        float maxSpan = fmaxf(extent.x, fmaxf(extent.y, extent.z));
        maxSpan *= 1.5f;
        eyeDist = maxSpan / (2 * tan((fov * 0.5f) * 0.01745329251994329576923690768489f));
    }
    // after VolumeReader::Crop / Resample returned rc: the reader's new texture, box and spacing, and a camera that sees all of it
    int AdoptVolume(int rc)
    {
        if (rc != 0) return rc;
        ClearRegion();
        volumeReader->CreateDeviceVolume(&deviceVolume);               // (the clips and the density scale stay)
        setup_volume(deviceVolume);
        ZoomToExtent();
        UpdateCamera();
        ReStartRender();
        return 0;
    }
    // the voxels that are segmented: the filtered copy when there is one, else the loaded ones (null unless KeepVoxels(true) was set)
    const uint16_t* SegVoxels() const { return filtered ? filtered : volumeReader->DeviceVoxels(); }
    // run a filter from SegVoxels() into a fresh buffer; on success that buffer becomes the filtered copy
    template <typename Call>
    int ReplaceFiltered(Call call)
    {
        if (!ready || !SegVoxels()) return -4;
        const int* dim = volumeReader->dim;
        uint16_t* out = (uint16_t*)svr_device_malloc((size_t)dim[0] * dim[1] * dim[2] * sizeof(uint16_t));
        if (!out) return -4;
        const int rc = call(out);
        svr_device_synchronize();
        if (rc != 0) { svr_device_free(out); return rc; }
        if (filtered) svr_device_free(filtered);
        filtered = out;
        return 0;
    }
    // a device array of n[0] x n[1] x n[2] elements to a MetaImage file with the spacing and the position of `vol`
    static int SaveDeviceArray(const std::string& filename, const void* device, int elem_type, size_t elem_size, const int n[3], const svr_volume& vol)
    {
        std::vector<uint8_t> host((size_t)n[0] * n[1] * n[2] * elem_size);
        if (int rc = svr_memcpy_d2h(host.data(), device, host.size())) return rc;
        const int32_t dims[3] = {n[0], n[1], n[2]};
        const double sp[3] = {vol.spacing.x, vol.spacing.y, vol.spacing.z};
        const double off[3] = {vol.bbox.vmin.x + 0.5 * sp[0], vol.bbox.vmin.y + 0.5 * sp[1], vol.bbox.vmin.z + 0.5 * sp[2]};
        return svr_mhd_write(filename.c_str(), host.data(), elem_type, dims, sp, off, 0);
    }
    // a device bit mask as u8 0 / 1
    static int SaveMask(const std::string& filename, const uint32_t* mask, const int n[3], const svr_volume& vol)
    {
        uint8_t* bytes = (uint8_t*)svr_device_malloc((size_t)n[0] * n[1] * n[2]);
        if (!bytes) return -4;
        const int32_t dims[3] = {n[0], n[1], n[2]};
        int rc = svr_region_mask_expand(mask, dims, 1, bytes);
        if (rc == 0) rc = SaveDeviceArray(filename, bytes, SVR_ELEM_U8, 1, n, vol);
        svr_device_synchronize();
        svr_device_free(bytes);
        return rc;
    }
    // a counting call, then an extraction into device arrays of the counted sizes, copied to the host
    template <typename Call>
    int ExtractSurface(Call call, svr_mesh_info* info_out)
    {
        svr_mesh_info info;
        haveSurface = false;
        int rc = call(nullptr, 0u, nullptr, 0u, &info);
        if (rc != 0) return rc;
        const size_t vbytes = (size_t)info.vertices * 3 * sizeof(int32_t), tbytes = (size_t)info.triangles * 3 * sizeof(uint32_t);
        surfaceVertices.assign((size_t)info.vertices * 3, 0);
        surfaceTriangles.assign((size_t)info.triangles * 3, 0u);
        if (info.vertices) {
            char* buf = (char*)svr_device_malloc(vbytes + tbytes);
            if (!buf) return -4;
            rc = call((int32_t*)buf, info.vertices, (uint32_t*)(buf + vbytes), info.triangles, &info);
            if (rc == 0) rc = svr_memcpy_d2h(surfaceVertices.data(), buf, vbytes);
            if (rc == 0 && tbytes) rc = svr_memcpy_d2h(surfaceTriangles.data(), buf + vbytes, tbytes);
            svr_device_free(buf);
        }
        haveSurface = rc == 0;
        if (info_out) *info_out = info;
        return rc;
    }
    void ClearRegion()
    {
        if (filtered) svr_device_free(filtered);
        filtered = nullptr;
        if (regionTex) svr_destroy_texture(regionTex);
        if (regionMask) svr_device_free(regionMask);
        if (regionWork) svr_device_free(regionWork);
        if (regionLabels) svr_device_free(regionLabels);
        regionTex = 0; regionMask = nullptr; regionWork = nullptr; regionLabels = nullptr; haveRegion = false; haveSeed = false; haveLabels = false;
        labelClasses = 0u;
        labelCount = 0u;
        ClearSeeds();                                  // (the strokes were voxels of the volume that goes)
    }
    // a device u16 volume of the loaded dimensions becomes the texture every renderer draws (ShowRegion, ShowRegionDistance)
    int ShowVoxels(const uint16_t* shown)
    {
        const int* dim = volumeReader->dim;
        const cudaTextureObject_t tex = svr_create_volume_texture(shown, dim[0], dim[1], dim[2], 1, SVR_LAYOUT_AUTO);    // (copies: `shown` is free afterwards)
        if (!tex) return svr_last_error_code() ? svr_last_error_code() : -4;
        svr_device_synchronize();                      // no frame in flight still reads the texture that goes
        if (regionTex) svr_destroy_texture(regionTex);
        regionTex = tex;
        deviceVolume.tex = tex;
        setup_volume(deviceVolume);
        ReStartRender();
        return 0;
    }
    // what the overlays read: the labels when they are current, else the mask
    svr_overlay_source RegionSource() const
    {
        return haveLabels ? svr_overlay_source{nullptr, regionLabels} : svr_overlay_source{regionMask, nullptr};
    }
    // a length in the spacing's units as the r2 of svr_region_ball
    static uint32_t LengthToR2(double length, double unit)
    {
        const double q = length / unit, r2 = std::floor(q * q);
        return r2 >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)r2;
    }
    // the scissor calls of the public section: slice == nullptr means the canvas's camera
    int Scissor(const svr_slice_params* slice, uint32_t w, uint32_t h, const std::vector<double>& polygon, int op, float thickness, svr_region_stats* stats)
    {
        const uint16_t* vox = SegVoxels();
        if (!ready || !vox) return -4;
        if (op != SVR_SCISSOR_ERASE_INSIDE && op != SVR_SCISSOR_ERASE_OUTSIDE && op != SVR_SCISSOR_FILL_INSIDE) return -3;
        if (!haveRegion && op != SVR_SCISSOR_FILL_INSIDE) return -4;
        if (polygon.size() < 6 || polygon.size() % 2 != 0 || polygon.size() / 2 > SVR_STENCIL_MAX_VERTICES || w == 0u || h == 0u) return -3;
        std::vector<int32_t> q8(polygon.size());
        for (size_t i = 0; i < polygon.size(); ++i) {
            const double v = std::nearbyint(polygon[i] * 256.0);
            if (!(std::fabs(v) <= (double)SVR_STENCIL_MAX_COORD)) return -3;
            q8[i] = (int32_t)v;
        }
        const int* dim = volumeReader->dim;
        if (!regionMask) regionMask = (uint32_t*)svr_device_malloc((size_t)svr_region_mask_words(dim[0], dim[1], dim[2]) * sizeof(uint32_t));
        if (!regionMask) return -4;
        uint32_t* stencil = (uint32_t*)svr_device_malloc((size_t)svr_region_mask_words((int)w, (int)h, 1) * sizeof(uint32_t));
        if (!stencil) return -4;
        const uint32_t count = (uint32_t)(polygon.size() / 2);
        svr_scissor_params p;
        svr_scissor_params_default(&p);
        p.op = haveRegion ? op : SVR_SCISSOR_SELECT;                  // (filling nothing: the prism itself)
        if (slice && thickness > 0.f) { p.depth_lo = -0.5f * thickness; p.depth_hi = 0.5f * thickness; }
        int rc = svr_stencil_polygon(q8.data(), &count, 1u, w, h, stencil);
        if (rc == 0)
            rc = slice ? svr_region_scissor_slice(regionMask, dim[0], dim[1], dim[2], &deviceVolume, slice, w, h, stencil, &p, regionMask)
                       : svr_region_scissor_camera(regionMask, dim[0], dim[1], dim[2], &deviceVolume, &camera, stencil, &p, regionMask);
        if (rc == 0) rc = svr_device_synchronize();                // the stencil is freed below
        svr_device_free(stencil);
        if (rc != 0) return rc;
        if (!haveRegion) { haveRegion = true; haveSeed = false; }
        haveLabels = false;                                        // (they were the parts of the mask that went)
        return stats ? svr_region_stats_of(vox, dim[0], dim[1], dim[2], 1, regionMask, stats) : 0;
    }
    // the second mask buffer, into which the clean-up calls write (their `out` must not overlap their input)
    bool WorkMask()
    {
        if (!ready || !SegVoxels() || !haveRegion) return false;
        const int* dim = volumeReader->dim;
        if (!regionWork) regionWork = (uint32_t*)svr_device_malloc((size_t)svr_region_mask_words(dim[0], dim[1], dim[2]) * sizeof(uint32_t));
        return regionWork != nullptr;
    }
    // after a clean-up call that returned rc: its result becomes the region mask
    int ReplaceRegion(int rc, svr_region_stats* stats)
    {
        if (rc != 0) return rc;
        std::swap(regionMask, regionWork);
        haveLabels = false;                            // (they were the parts of the mask that went)
        if (!stats) return 0;
        const int* dim = volumeReader->dim;
        return svr_region_stats_of(SegVoxels(), dim[0], dim[1], dim[2], 1, regionMask, stats);
    }
    // label the region, tabulate its components, keep those of at least min_voxels voxels among the largest_k largest (0 = no limit)
    int SelectRegionParts(uint32_t min_voxels, uint32_t largest_k, int connectivity, svr_region_stats* stats)
    {
        if (!WorkMask()) return -4;
        const int* dim = volumeReader->dim;
        uint32_t* labels = (uint32_t*)svr_device_malloc((size_t)dim[0] * dim[1] * dim[2] * sizeof(uint32_t));
        if (!labels) return -4;
        uint32_t count = 0u, kept = 0u;
        int rc = svr_region_label(regionMask, dim[0], dim[1], dim[2], connectivity, labels, &count);
        if (rc == 0 && count == 0u) {                                           // an empty region has no component: it stays empty
            svr_device_free(labels);
            return stats ? svr_region_stats_of(SegVoxels(), dim[0], dim[1], dim[2], 1, regionMask, stats) : 0;
        }
        svr_region_component* table = rc == 0 ? (svr_region_component*)svr_device_malloc((size_t)count * sizeof(svr_region_component)) : nullptr;
        if (rc == 0 && !table) rc = -4;
        if (rc == 0) rc = svr_region_label_table(labels, nullptr, dim[0], dim[1], dim[2], 1, count, table);
        if (rc == 0) rc = svr_region_select_by_size(labels, dim[0], dim[1], dim[2], count, table, min_voxels, largest_k, regionWork, &kept);
        if (table) svr_device_free(table);                                      // (select_by_size synchronised the stream)
        svr_device_free(labels);
        return ReplaceRegion(rc, stats);
    }
    void UpdateCamera()                                                         // canvas.cpp:178-188
    {
        const glm::vec3 u = view[0], v = view[1], w = view[2];
        const glm::vec3 pos = w * eyeDist - u * cameraTranslate.x - v * cameraTranslate.y;
        camera.Setup(pos, u, v, w, fov, apeture, focalLength, exposure, WIDTH, HEIGHT);
        setup_camera(camera);
    }

    bool ready = false;
    glm::u8vec4* img = nullptr;
    float exposure = 1.f, apeture = 0.f, fov = 45.f, focalLength = 1.f, eyeDist = 0.f;
    glm::vec2 cameraTranslate;
    glm::vec3 view[3];                             // rows of the reference's viewMat: camera u, v, w
    RenderParams renderParams;
    cudaCamera camera;
    cudaVolume deviceVolume;
    cudaTransferFunction transferFunction;
    RenderMode renderMode = RENDER_MODE_RAYCASTING;
    uint32_t* regionMask = nullptr;                // GrowRegion's bit mask (device)
    uint32_t* regionWork = nullptr;                // the other mask buffer of the clean-up calls
    uint32_t* regionLabels = nullptr;              // LabelRegion's parts of the region (device, uint32 per voxel); freed with regionMask
    bool haveLabels = false;                       // false once anything replaces the region
    uint32_t labelClasses = 0u;                    // > 0: the labels are the classes 1 .. labelClasses of GrowFromSeeds
    uint32_t labelCount = 0u;                      // the largest label of the current label map (parts or classes): SmoothRegionParts
    uint32_t* seedMarkers = nullptr;               // AddSeed's marker map (device, uint32 per voxel): 0 = no stroke, else the class
    uint32_t seedMaxClass = 0u;                    // the largest class painted on it
    int32_t regionSeed[3] = {0, 0, 0};             // GrowRegion's seed voxel and connectivity, for DetachRegion
    int regionConnectivity = 6;
    bool haveSeed = false;                         // false after ThresholdRegion: the region then comes from no pick
    cudaTextureObject_t regionTex = 0;             // ShowRegion's masked volume
    bool haveRegion = false;
    uint16_t* filtered = nullptr;                  // MedianVolume / SmoothVolume's copy of the voxels (device)
    std::vector<int32_t> surfaceVertices;          // ExtractRegionSurface / ExtractIsoSurface's mesh (host)
    std::vector<uint32_t> surfaceTriangles;
    bool haveSurface = false;
    svr_projection_params projection = {SVR_PROJ_MIP, 0u, 0.5f, 0.f, 1.f};
    svr_slice_params slice = {{0.f, 0.f, 0.f}, {1.f, 0.f, 0.f}, {0.f, 1.f, 0.f}, 0.f, 1.f, SVR_SLAB_MIP, 0u, 0.f, 1.f};
};

#endif  // SUNVOLUMERENDER_CANVAS_HPP
