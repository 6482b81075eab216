// sdf3d.hpp -- C++ host/scene API over the C-ABI of include/sdf_abi.h.
//
// Mirrors the shape of the reference host program (/root/reference/Code/src/
// main.cpp): objects created once (main.cpp:48-56), the device program set up
// once (:67-77), a per-frame draw in a loop (:87-98) and explicit cleanup
// (:103-107).  Where the reference hard-codes the scene, camera, light and
// material inside the fragment shader (voxel_fragment.frag:178-189), this API
// takes them as values; sdf::Frame::reference() reproduces the hard-coded ones.
//
// Header-only; link against libsdf3d.so and amdhip64.  Errors are reported as
// sdf::Error exceptions on this side of the boundary (the C-ABI itself never
// throws).
#pragma once

#include <hip/hip_runtime.h>

#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "sdf_abi.h"

namespace sdf {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& what)
      : std::runtime_error(what + ": " + sdf_strerror(c)), code(c) {}
};

inline void check(int rc, const char* what) {
  if (rc != SDF_OK) throw Error(rc, what);
}
inline void check_hip(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
// The loaded libsdf3d must implement the ABI these headers describe (struct
// layouts and signatures change with SDF_ABI_VERSION); checked once by every
// object that calls into it.
inline void check_abi() {
  static const int v = sdf_abi_version();
  if (v != SDF_ABI_VERSION)
    throw Error(SDF_E_UNSUPPORTED, "libsdf3d ABI " + std::to_string(v) + " != headers' " +
                                       std::to_string(SDF_ABI_VERSION));
}

// Scene builder: primitives combined left to right into d (d starts at +INF,
// voxel_fragment.frag:75).
class Scene {
 public:
  Scene() { std::memset(&s_, 0, sizeof(s_)); s_.kind = SDF_SCENE_PRIMITIVES; s_.bulb_scale = 1.0f;
            s_.bulb_iterations = 12; s_.bulb_bailout = 2.0f; }
  explicit Scene(const sdf_scene& s) : s_(s) {}

  Scene& sphere(float cx, float cy, float cz, float r, int op = SDF_OP_UNION, float k = 0) {
    return add(SDF_PRIM_SPHERE, op, k, {cx, cy, cz, r});
  }
  Scene& plane(float nx, float ny, float nz, float h, int op = SDF_OP_UNION, float k = 0) {
    return add(SDF_PRIM_PLANE, op, k, {nx, ny, nz, h});
  }
  Scene& box(float cx, float cy, float cz, float hx, float hy, float hz, int op = SDF_OP_UNION,
             float k = 0) {
    return add(SDF_PRIM_BOX, op, k, {cx, cy, cz, hx, hy, hz});
  }
  Scene& round_box(float cx, float cy, float cz, float hx, float hy, float hz, float r,
                   int op = SDF_OP_UNION, float k = 0) {
    return add(SDF_PRIM_ROUND_BOX, op, k, {cx, cy, cz, hx, hy, hz, r});
  }
  Scene& torus(float cx, float cy, float cz, float R, float r, int op = SDF_OP_UNION,
               float k = 0) {
    return add(SDF_PRIM_TORUS, op, k, {cx, cy, cz, R, r});
  }
  Scene& capsule(float ax, float ay, float az, float bx, float by, float bz, float r,
                 int op = SDF_OP_UNION, float k = 0) {
    return add(SDF_PRIM_CAPSULE, op, k, {ax, ay, az, bx, by, bz, r});
  }
  Scene& cylinder(float cx, float cy, float cz, float r, float half_h, int op = SDF_OP_UNION,
                  float k = 0) {
    return add(SDF_PRIM_CYLINDER, op, k, {cx, cy, cz, r, half_h});
  }
  Scene& mandelbulb(float cx, float cy, float cz, float scale, int iterations = 12,
                    float bailout = 2.0f) {
    s_.kind = SDF_SCENE_MANDELBULB;
    s_.count = 0;
    s_.bulb_center[0] = cx; s_.bulb_center[1] = cy; s_.bulb_center[2] = cz;
    s_.bulb_scale = scale; s_.bulb_iterations = iterations; s_.bulb_bailout = bailout;
    return *this;
  }
  const sdf_scene& raw() const { return s_; }
  sdf_scene& raw() { return s_; }

 private:
  Scene& add(int kind, int op, float k, std::initializer_list<float> p) {
    if (s_.count >= SDF_MAX_PRIMS) throw Error(SDF_E_INVALID_ARG, "Scene: too many primitives");
    sdf_primitive& pr = s_.prims[s_.count++];
    std::memset(&pr, 0, sizeof(pr));
    pr.kind = kind; pr.op = op; pr.k = k;
    int i = 0;
    for (float v : p) pr.p[i++] = v;
    return *this;
  }
  sdf_scene s_;
};

// Everything one frame needs besides the output.
struct Frame {
  sdf_scene scene;
  sdf_camera camera;
  sdf_light light;
  sdf_material material;
  sdf_params params;

  // The reference shader's hard-coded frame (voxel_fragment.frag:15-23,
  // :54-81, :178-189, :205) at width x height (<= 0: 800 x 600, main.cpp:4-5).
  static Frame reference(int width = 0, int height = 0) {
    check_abi();
    Frame f;
    check(sdf_defaults(&f.scene, &f.camera, &f.light, &f.material, &f.params, width, height),
          "sdf_defaults");
    return f;
  }
  // Orbit the camera about the origin: V_mat = Rx(pitch) * Ry(yaw), column-major
  // (the reference gets V_mat from Neutrino's arcball, main.cpp:93-94).
  Frame& orbit(float yaw_deg, float pitch_deg) {
    const double y = yaw_deg * M_PI / 180.0, p = pitch_deg * M_PI / 180.0;
    const double cy = std::cos(y), sy = std::sin(y), cp = std::cos(p), sp = std::sin(p);
    // rows of Rx*Ry
    const double m[4][4] = {{cy, 0, sy, 0}, {sp * sy, cp, -sp * cy, 0},
                            {-cp * sy, sp, cp * cy, 0}, {0, 0, 0, 1}};
    for (int c = 0; c < 4; ++c)
      for (int r = 0; r < 4; ++r) camera.view[c * 4 + r] = static_cast<float>(m[r][c]);
    return *this;
  }
  // Sub-samples per axis (params.samples): 1 one ray per pixel, 2 or 4 fused
  // supersampling -- every pixel the box-filtered S x S sub-samples, resolved
  // in the kernel (sdf_abi.h "Supersampling"); the framebuffer stays W x H.
  // Renderer::render's `steps` then takes S H x S W int2.
  Frame& supersample(int samples) {
    params.samples = samples;
    return *this;
  }
  // The material table of a shading call: `v`, or where it is empty the
  // frame's material on every primitive (once for a Mandelbulb).
  std::vector<sdf_material> table(const std::vector<sdf_material>& v) const {
    const size_t n = scene.kind == SDF_SCENE_PRIMITIVES ? static_cast<size_t>(scene.count) : 1;
    return v.empty() ? std::vector<sdf_material>(n, material) : v;
  }
};

// Arcball navigation producing V_mat: the reference
// drives V_mat from Neutrino's mouse and gamepad navigation with these rates
// (main.cpp:37-45: orbit 1 rev/s, pan 5 m/s, decay 1.25 s; gamepad orbit 1,
// pan 1, decay 1.25, deadzone 0.30), called once per frame (:93-94).
// Neutrino's implementation is not vendored, so the dynamics are this
// framework's own (parity unpinned), identical to sdf3d_amd/camera.py (the
// tests compare the two sequences bit for bit):
//   * while a mouse button drags, orbit (or pan) velocity = rate * motion / dt;
//     released, the velocity decays by exp(-dt / decay_time) per update;
//   * a gamepad stick outside the deadzone sets the velocity to
//     rate * 2 pi (orbit, rev/s) or rate (pan) times the stick value rescaled
//     from [deadzone, 1] to [0, 1]; inside it, the velocity decays;
//   * pitch is clamped to [-pi/2, pi/2]; V_mat = T(pan) * Rx(pitch) * Ry(yaw).
// All arithmetic in double, the matrix rounded to float once.
class Arcball {
 public:
  struct Rates {
    double orbit_rate = 1.0, pan_rate = 5.0, decay_time = 1.25;     // mouse, main.cpp:37-39
    double pad_orbit_rate = 1.0, pad_pan_rate = 1.0, pad_decay_time = 1.25,
           pad_deadzone = 0.30;                                       // gamepad, main.cpp:42-45
  };
  Arcball() = default;
  explicit Arcball(const Rates& r) : r_(r) {}

  // Mouse: pointer motion (dx, dy) in normalised screen units over dt seconds.
  void mouse(double dt, double dx, double dy, bool orbit, bool pan) {
    if (!(dt > 0)) return;
    if (orbit) vyaw_ = r_.orbit_rate * dx / dt, vpitch_ = r_.orbit_rate * dy / dt;
    if (pan) vpx_ = r_.pan_rate * dx / dt, vpy_ = r_.pan_rate * dy / dt;
    integrate(dt, !orbit, !pan, r_.decay_time);
  }
  // Gamepad: left stick (lx, ly) orbits, right stick (rx, ry) pans, in [-1, 1].
  void gamepad(double dt, double lx, double ly, double rx, double ry) {
    if (!(dt > 0)) return;
    const double ax = dead(lx), ay = dead(ly), bx = dead(rx), by = dead(ry);
    const bool orbit = ax != 0.0 || ay != 0.0, pan = bx != 0.0 || by != 0.0;
    const double two_pi = 2.0 * M_PI;
    if (orbit) vyaw_ = r_.pad_orbit_rate * two_pi * ax, vpitch_ = r_.pad_orbit_rate * two_pi * ay;
    if (pan) vpx_ = r_.pad_pan_rate * bx, vpy_ = r_.pad_pan_rate * by;
    integrate(dt, !orbit, !pan, r_.pad_decay_time);
  }
  // V_mat, column-major float (sdf_camera.view).
  void view(float* out16) const {
    const double cy = std::cos(yaw_), sy = std::sin(yaw_), cp = std::cos(pitch_),
                 sp = std::sin(pitch_);
    const double m[4][4] = {{cy, 0, sy, pan_x_}, {sp * sy, cp, -sp * cy, pan_y_},
                            {-cp * sy, sp, cp * cy, 0}, {0, 0, 0, 1}};
    for (int c = 0; c < 4; ++c)
      for (int r = 0; r < 4; ++r) out16[c * 4 + r] = static_cast<float>(m[r][c]);
  }
  void apply(Frame& f) const { view(f.camera.view); }
  double yaw() const { return yaw_; }
  double pitch() const { return pitch_; }

 private:
  double dead(double a) const {
    const double z = r_.pad_deadzone, m = std::fabs(a);
    if (!(m > z)) return 0.0;
    return std::copysign(std::min((m - z) / (1.0 - z), 1.0), a);
  }
  void integrate(double dt, bool decay_orbit, bool decay_pan, double tau) {
    yaw_ += vyaw_ * dt;
    pitch_ = std::max(-M_PI / 2, std::min(M_PI / 2, pitch_ + vpitch_ * dt));
    pan_x_ += vpx_ * dt;
    pan_y_ += vpy_ * dt;
    if (decay_orbit || decay_pan) {
      const double k = tau > 0 ? std::exp(-dt / tau) : 0.0;
      if (decay_orbit) vyaw_ *= k, vpitch_ *= k;
      if (decay_pan) vpx_ *= k, vpy_ *= k;
    }
  }
  Rates r_;
  double yaw_ = 0, pitch_ = 0, pan_x_ = 0, pan_y_ = 0;
  double vyaw_ = 0, vpitch_ = 0, vpx_ = 0, vpy_ = 0;
};

// n (<= SDF_MAX_PRIMS) distinct materials, one per primitive, for
// Renderer::render(f, lights, light_flags, materials): a fixed table (the
// Python package's scenes.palette), amb = dif = the entry's colour, ref = its
// reflectance on every channel, all with the same shininess
// (sdf_render_materials keeps the exponent frame-wide).
inline std::vector<sdf_material> palette(int n, float shininess = 12.0f) {
  static const float kPalette[SDF_MAX_PRIMS][4] = {
      {0.75f, 0.75f, 0.72f, 0.2f}, {0.85f, 0.15f, 0.1f, 0.5f}, {0.1f, 0.55f, 0.85f, 0.5f},
      {0.95f, 0.7f, 0.1f, 0.6f},   {0.2f, 0.7f, 0.25f, 0.4f},  {0.6f, 0.25f, 0.75f, 0.5f},
      {0.95f, 0.45f, 0.1f, 0.5f},  {0.1f, 0.75f, 0.7f, 0.6f},  {0.9f, 0.35f, 0.6f, 0.4f},
      {0.35f, 0.3f, 0.85f, 0.5f},  {0.6f, 0.8f, 0.15f, 0.4f},  {0.55f, 0.35f, 0.2f, 0.3f},
      {0.25f, 0.25f, 0.3f, 0.7f},  {0.95f, 0.9f, 0.8f, 0.3f},  {0.0f, 0.2f, 0.8f, 0.5f},
      {0.5f, 0.05f, 0.15f, 0.6f}};
  if (n < 0 || n > SDF_MAX_PRIMS) throw Error(SDF_E_INVALID_ARG, "palette: at most 16 entries");
  std::vector<sdf_material> out(static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) {
    sdf_material m{};
    for (int c = 0; c < 3; ++c) {
      m.amb[c] = m.dif[c] = kPalette[i][c];
      m.ref[c] = kPalette[i][3];
    }
    m.shininess = shininess;
    out[static_cast<size_t>(i)] = m;
  }
  return out;
}

// The default environment of sdf_render_env (the Python package's
// scenes.sky): a gradient from the horizon up to the zenith and down to the
// ground, a glow around the sun (its direction normalised in double precision
// and rounded to float), every colour component in [0, 1]; the fog fields
// hold the horizon's colour and the range 0 .. 1 until sdf::fog sets them.
// `flags`: the SDF_ENV_* bits to set.
inline sdf_environment sky(int32_t flags = SDF_ENV_SKY | SDF_ENV_SUN) {
  static const float kHorizon[3] = {0.72f, 0.80f, 0.90f}, kZenith[3] = {0.18f, 0.36f, 0.72f},
                     kGround[3] = {0.30f, 0.27f, 0.24f}, kSunColor[3] = {1.0f, 0.9f, 0.6f};
  static const double kSunDir[3] = {-0.4, 0.6, 0.7};
  const double n = std::sqrt((kSunDir[0] * kSunDir[0] + kSunDir[1] * kSunDir[1]) +
                             kSunDir[2] * kSunDir[2]);
  sdf_environment e{};
  for (int c = 0; c < 3; ++c) {
    e.horizon[c] = e.fog_color[c] = kHorizon[c];
    e.zenith[c] = kZenith[c];
    e.ground[c] = kGround[c];
    e.sun_dir[c] = static_cast<float>(kSunDir[c] / n);
    e.sun_color[c] = kSunColor[c];
  }
  e.sun_exponent = 64.0f;
  e.fog_start = 0.0f;
  e.fog_end = 1.0f;
  e.flags = flags;
  return e;
}
// `env` with linear distance fog from `start` to `end` switched on, in its
// present fog colour (the horizon's after sdf::sky) or in `rgb`.
inline sdf_environment fog(sdf_environment env, float start, float end,
                           const float* rgb = nullptr) {
  env.fog_start = start;
  env.fog_end = end;
  if (rgb)
    for (int c = 0; c < 3; ++c) env.fog_color[c] = rgb[c];
  env.flags |= SDF_ENV_FOG;
  return env;
}

// Owns a device framebuffer and renders frames into it on one HIP stream.
// The buffer holds width x height pixels of up to 16 bytes (any sdf_format).
class Renderer {
 public:
  Renderer(int width, int height, hipStream_t stream = nullptr)
      : w_(width), h_(height), stream_(stream) {
    check_abi();
    check_hip(hipMalloc(&rgba_, size_t(w_) * h_ * 16), "hipMalloc");
  }
  ~Renderer() { if (rgba_) (void)hipFree(rgba_); }
  Renderer(const Renderer&) = delete;
  Renderer& operator=(const Renderer&) = delete;

  // One frame (the reference's gl->plot(sh, proj_mode), main.cpp:95).
  void render(const Frame& f, const sdf_tiling* tiling = nullptr, int32_t* steps = nullptr) {
    if (f.params.width != w_ || f.params.height != h_)
      throw Error(SDF_E_INVALID_ARG, "Renderer: frame size differs from framebuffer");
    check(sdf_render(&f.scene, &f.camera, &f.light, &f.material, &f.params, tiling, rgba_, steps,
                     stream_),
          "sdf_render");
  }
  // The frame under `lights` (1 .. SDF_MAX_LIGHTS, f.light is ignored) with
  // light_flags (SDF_LIGHTS_COLOR: every light scaled by its colour):
  // sdf_render_lights, the surface traced once for all of them.
  void render(const Frame& f, const std::vector<sdf_light>& lights, int32_t light_flags = 0,
              const sdf_tiling* tiling = nullptr, int32_t* steps = nullptr,
              sdf_schedule* schedule = nullptr) {
    if (f.params.width != w_ || f.params.height != h_)
      throw Error(SDF_E_INVALID_ARG, "Renderer: frame size differs from framebuffer");
    check(sdf_render_lights(&f.scene, &f.camera, lights.data(),
                            static_cast<int32_t>(lights.size()), light_flags, &f.material,
                            &f.params, tiling, rgba_, steps, schedule, stream_),
          "sdf_render_lights");
  }
  // The frame under `lights` with a material per primitive of the scene (one
  // for a Mandelbulb; f.material is ignored), blended along the CSG fold at
  // every pixel: sdf_render_materials.  sdf::palette(n) gives n distinct ones.
  void render(const Frame& f, const std::vector<sdf_light>& lights, int32_t light_flags,
              const std::vector<sdf_material>& materials, const sdf_tiling* tiling = nullptr,
              int32_t* steps = nullptr, sdf_schedule* schedule = nullptr) {
    if (f.params.width != w_ || f.params.height != h_)
      throw Error(SDF_E_INVALID_ARG, "Renderer: frame size differs from framebuffer");
    check(sdf_render_materials(&f.scene, &f.camera, lights.data(),
                               static_cast<int32_t>(lights.size()), light_flags,
                               materials.data(), static_cast<int32_t>(materials.size()),
                               &f.params, tiling, rgba_, steps, schedule, stream_),
          "sdf_render_materials");
  }
  // The materials frame with mirror reflections: up to SDF_MAX_BOUNCES
  // bounces per pixel, each surface's blended ref times reflect.strength
  // weighting what it reflects (sdf_render_reflect; reflect.layer = -1 is the
  // composite).  An empty `materials` gives every primitive f.material.
  void render(const Frame& f, const std::vector<sdf_light>& lights, int32_t light_flags,
              const std::vector<sdf_material>& materials, const sdf_reflect& reflect,
              const sdf_tiling* tiling = nullptr, int32_t* steps = nullptr,
              sdf_schedule* schedule = nullptr) {
    if (f.params.width != w_ || f.params.height != h_)
      throw Error(SDF_E_INVALID_ARG, "Renderer: frame size differs from framebuffer");
    const std::vector<sdf_material> m = f.table(materials);
    check(sdf_render_reflect(&f.scene, &f.camera, lights.data(),
                             static_cast<int32_t>(lights.size()), light_flags, m.data(),
                             static_cast<int32_t>(m.size()), &reflect, &f.params, tiling, rgba_,
                             steps, schedule, stream_),
          "sdf_render_reflect");
  }
  // The reflect frame with an environment: a sky for the rays that leave the
  // scene and linear distance fog (sdf_render_env; sdf::sky() and sdf::fog()
  // make one).  reflect.bounces = 0 is legal: one layer.
  void render(const Frame& f, const std::vector<sdf_light>& lights, int32_t light_flags,
              const std::vector<sdf_material>& materials, const sdf_reflect& reflect,
              const sdf_environment& env, const sdf_tiling* tiling = nullptr,
              int32_t* steps = nullptr, sdf_schedule* schedule = nullptr) {
    if (f.params.width != w_ || f.params.height != h_)
      throw Error(SDF_E_INVALID_ARG, "Renderer: frame size differs from framebuffer");
    const std::vector<sdf_material> m = f.table(materials);
    check(sdf_render_env(&f.scene, &f.camera, lights.data(), static_cast<int32_t>(lights.size()),
                         light_flags, m.data(), static_cast<int32_t>(m.size()), &reflect, &env,
                         &f.params, tiling, rgba_, steps, schedule, stream_),
          "sdf_render_env");
  }
  // Blocking copy of an RGBA32F framebuffer (row 0 = bottom, GL order).
  std::vector<float> download() const {
    std::vector<float> out(size_t(w_) * h_ * 4);
    copy_out(out.data(), out.size() * sizeof(float));
    return out;
  }
  // Blocking copy of the framebuffer bytes of any format.
  std::vector<unsigned char> download_bytes(int format) const {
    const int bpp = sdf_format_bytes(format);
    if (bpp < 0) throw Error(bpp, "download_bytes");
    std::vector<unsigned char> out(size_t(w_) * h_ * bpp);
    copy_out(out.data(), out.size());
    return out;
  }
  float* device_rgba() const { return rgba_; }
  int width() const { return w_; }
  int height() const { return h_; }

 private:
  void copy_out(void* dst, size_t bytes) const {
    check_hip(hipMemcpyAsync(dst, rgba_, bytes, hipMemcpyDeviceToHost, stream_),
              "hipMemcpyAsync");
    check_hip(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  }
  int w_, h_;
  hipStream_t stream_;
  float* rgba_ = nullptr;
};

// ---- queries (sdf_abi.h "Queries") -------------------------------------------
// Rays and points asked of a frame's scene with the frame's march parameters,
// normal mode, precision and dispatch.  Every pointer is device memory;
// `origins`, `dirs` and `points` hold n x 3 packed floats; any member of `hits`
// may be null, not all.  Asynchronous on `stream`.
inline void trace(const Frame& f, const float* origins, const float* dirs, int64_t n,
                  const sdf_hits& hits, hipStream_t stream = nullptr) {
  check(sdf_trace(&f.scene, &f.params, origins, dirs, n, &hits, stream), "sdf_trace");
}
// The rays sdf_render marches: entry y * width + x is pixel (x, y)'s (row 0 =
// bottom), so hits.t is a depth map and hits.prim a segmentation map.
inline void trace_camera(const Frame& f, const sdf_hits& hits, hipStream_t stream = nullptr) {
  check(sdf_trace_camera(&f.scene, &f.camera, &f.params, &hits, stream), "sdf_trace_camera");
}
// The scene's signed distance (and, with `normal`, its normal) at n points.
inline void sample(const Frame& f, const float* points, int64_t n, float* dist,
                   float* normal = nullptr, hipStream_t stream = nullptr) {
  check(sdf_sample(&f.scene, &f.params, points, n, dist, normal, stream), "sdf_sample");
}

// What lies under pixel (x, y) of the frame (row 0 = bottom): the march's
// distance and iteration count, the primitive that owns the hit (-1: the ray
// left the scene) and the normal there.  Blocking; traces the frame's rays
// with sdf_trace_camera and reads one pixel back.  An interactive host that
// picks often keeps the maps of trace_camera instead.
struct Hit {
  float t;
  int32_t steps;
  int32_t prim;
  float normal[3];
};
inline Hit pick(const Frame& f, int x, int y, hipStream_t stream = nullptr) {
  check_abi();
  const int w = f.params.width, h = f.params.height;
  if (x < 0 || y < 0 || x >= w || y >= h) throw Error(SDF_E_INVALID_ARG, "pick: pixel outside the frame");
  const size_t n = size_t(w) * h, i = size_t(y) * w + x;
  char* buf = nullptr;
  check_hip(hipMalloc(reinterpret_cast<void**>(&buf), n * 24), "hipMalloc");
  sdf_hits hits;
  hits.t = reinterpret_cast<float*>(buf);
  hits.steps = reinterpret_cast<int32_t*>(buf + n * 4);
  hits.prim = reinterpret_cast<int32_t*>(buf + n * 8);
  hits.normal = reinterpret_cast<float*>(buf + n * 12);
  Hit out{};
  const int rc = sdf_trace_camera(&f.scene, &f.camera, &f.params, &hits, stream);
  hipError_t e = hipSuccess;
  if (rc == SDF_OK) {
    const hipMemcpyKind k = hipMemcpyDeviceToHost;
    e = hipMemcpyAsync(&out.t, hits.t + i, 4, k, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&out.steps, hits.steps + i, 4, k, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&out.prim, hits.prim + i, 4, k, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out.normal, hits.normal + 3 * i, 12, k, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
  }
  (void)hipFree(buf);
  check(rc, "sdf_trace_camera");
  check_hip(e, "pick");
  return out;
}

// ---- caller-supplied rays (sdf_abi.h "Rays") -----------------------------------
// The shading pipeline on rays of the caller's own camera model: ray i of
// `origins` / `dirs` (device, n x 3 packed floats; `unit`: the directions are
// unit vectors used as given, SDF_RAYS_UNIT) gives pixel i of `rgba` (device, n
// pixels of f.params.output_format) and, when non-null, entry i of `steps` (n
// int2).  An empty `materials` gives every primitive f.material; `reflect` and
// `env` may be null (no bounce, no environment).  The frame's camera, size and
// samples play no part.  A wave shades 64 consecutive rays: order them in
// coherent groups of 64.  Asynchronous on `stream`.
inline void render_rays(const Frame& f, const std::vector<sdf_light>& lights, int32_t light_flags,
                        const std::vector<sdf_material>& materials, const sdf_reflect* reflect,
                        const sdf_environment* env, const float* origins, const float* dirs,
                        int64_t n, bool unit, void* rgba, int32_t* steps = nullptr,
                        hipStream_t stream = nullptr) {
  const std::vector<sdf_material> m = f.table(materials);
  const sdf_rays rays = {origins, dirs, n, unit ? SDF_RAYS_UNIT : 0, 0};
  check(sdf_render_rays(&f.scene, lights.data(), static_cast<int32_t>(lights.size()), light_flags,
                        m.data(), static_cast<int32_t>(m.size()), reflect, env, &f.params, &rays,
                        rgba, steps, stream),
        "sdf_render_rays");
}
// The rays sdf_render marches for the frame: entry y * width + x of `origins`
// and `dirs` (device, width * height x 3 packed floats; either may be null) is
// pixel (x, y)'s eye and unit direction (row 0 = bottom).
inline void camera_rays(const Frame& f, float* origins, float* dirs,
                        hipStream_t stream = nullptr) {
  check(sdf_camera_rays(&f.camera, &f.params, origins, dirs, stream), "sdf_camera_rays");
}

// ---- gradients (sdf_abi.h "Gradients") -----------------------------------------
// The scene function's analytic gradients at n points (device, n x 3 packed
// floats) with the weights `upstream` (device, n; null: every weight 1).  Returns
// the 256 parameter sums, row i the sixteen slots of sdf_primitive i (2: k, 4 +
// j: p[j]); `dist` (device, n) and `grad_points` (device, 3 n: weight x df/dp) are
// written when non-null.  Allocates its own workspace.  Blocking.
inline std::array<float, 16 * SDF_MAX_PRIMS> sample_grad(
    const Frame& f, const float* points, int64_t n, const float* upstream = nullptr,
    float* dist = nullptr, float* grad_points = nullptr, hipStream_t stream = nullptr) {
  check_abi();
  check(sdf_validate_grad(&f.scene, &f.params), "sdf_validate_grad");
  const int64_t bytes = sdf_grad_workspace_bytes(n);
  if (bytes < 0) check(static_cast<int>(bytes), "sdf_grad_workspace_bytes");
  std::array<float, 16 * SDF_MAX_PRIMS> sums{};
  if (n == 0) return sums;
  char* buf = nullptr;   // the sums, then the workspace (16-byte aligned: 1024 bytes in)
  int rc = SDF_OK;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&buf), sizeof(sums) + size_t(bytes));
  if (e == hipSuccess) {
    const sdf_grad_out out = {dist, grad_points, reinterpret_cast<float*>(buf)};
    rc = sdf_sample_grad(&f.scene, &f.params, points, n, upstream, &out, buf + sizeof(sums), bytes,
                         stream);
    if (rc == SDF_OK)
      e = hipMemcpyAsync(sums.data(), buf, sizeof(sums), hipMemcpyDeviceToHost, stream);
    if (rc == SDF_OK && e == hipSuccess) e = hipStreamSynchronize(stream);
  }
  (void)hipFree(buf);
  check(rc, "sdf_sample_grad");
  check_hip(e, "sample_grad");
  return sums;
}

// ---- isosurface meshes (sdf_abi.h "Meshes") -----------------------------------
// The level set f(p) = grid.iso of the frame's scene inside `grid` as an
// indexed triangle mesh on the host: sdf_mesh_count, buffers sized from its
// counts, sdf_mesh_emit, and the copies back.  Blocking.  `normals`: one normal
// per vertex (sdf_sample's); `prims`: the primitive that owns each vertex;
// `sharp`: vertices on the scene's edges and corners (sdf_mesh_emit_sharp,
// "Sharp meshes"; nullptr: the plain surface-nets vertices).
struct Mesh {
  std::vector<float> verts;     // 3 per vertex
  std::vector<int32_t> tris;    // 3 vertex numbers per triangle
  std::vector<float> normals;   // 3 per vertex, or empty
  std::vector<int32_t> prims;   // 1 per vertex, or empty
  int64_t counts[4];            // vertices, triangles, bricks evaluated, bricks in all
};
inline Mesh extract_mesh(const Frame& f, const sdf_grid& grid, bool normals = false,
                         bool prims = false, hipStream_t stream = nullptr,
                         const sdf_mesh_sharp* sharp = nullptr) {
  check_abi();
  check(sdf_validate_mesh_sharp(&f.scene, &f.params, &grid, sharp), "sdf_validate_mesh_sharp");
  const int64_t bytes = sdf_mesh_workspace_bytes(&grid);
  if (bytes < 0) check(static_cast<int>(bytes), "sdf_mesh_workspace_bytes");
  Mesh m{};
  char *ws = nullptr, *buf = nullptr;
  int64_t* counts = nullptr;
  int rc = SDF_OK;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&ws), size_t(bytes));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&counts), 32);
  if (e == hipSuccess) {
    rc = sdf_mesh_count(&f.scene, &f.params, &grid, ws, bytes, counts, stream);
    if (rc == SDF_OK) e = hipMemcpyAsync(m.counts, counts, 32, hipMemcpyDeviceToHost, stream);
    if (rc == SDF_OK && e == hipSuccess) e = hipStreamSynchronize(stream);
  }
  if (rc == SDF_OK && e == hipSuccess && m.counts[0] > 0) {
    const size_t nv = size_t(m.counts[0]), nt = size_t(m.counts[1]);
    // verts | tris | normals | prims, every part a multiple of 4 bytes
    const size_t ov = 0, ot = ov + nv * 12, on = ot + nt * 12, op = on + (normals ? nv * 12 : 0),
                 end = op + (prims ? nv * 4 : 0);
    e = hipMalloc(reinterpret_cast<void**>(&buf), end);
    if (e == hipSuccess) {
      sdf_mesh_out out{};
      out.verts = reinterpret_cast<float*>(buf + ov);
      out.max_verts = m.counts[0];
      out.tris = nt ? reinterpret_cast<int32_t*>(buf + ot) : nullptr;
      out.max_tris = m.counts[1];
      out.normal = normals ? reinterpret_cast<float*>(buf + on) : nullptr;
      out.prim = prims ? reinterpret_cast<int32_t*>(buf + op) : nullptr;
      rc = sdf_mesh_emit_sharp(&f.scene, &f.params, &grid, sharp, ws, bytes, &out, stream);
      if (rc == SDF_OK) e = hipStreamSynchronize(stream);
      const hipMemcpyKind k = hipMemcpyDeviceToHost;
      if (rc == SDF_OK && e == hipSuccess) {
        m.verts.resize(nv * 3);
        m.tris.resize(nt * 3);
        if (normals) m.normals.resize(nv * 3);
        if (prims) m.prims.resize(nv);
        e = hipMemcpy(m.verts.data(), buf + ov, nv * 12, k);
        if (e == hipSuccess && nt) e = hipMemcpy(m.tris.data(), buf + ot, nt * 12, k);
        if (e == hipSuccess && normals) e = hipMemcpy(m.normals.data(), buf + on, nv * 12, k);
        if (e == hipSuccess && prims) e = hipMemcpy(m.prims.data(), buf + op, nv * 4, k);
      }
    }
  }
  (void)hipFree(buf);
  (void)hipFree(counts);
  (void)hipFree(ws);
  check(rc, "sdf_mesh_count / sdf_mesh_emit_sharp");
  check_hip(e, "extract_mesh");
  return m;
}
// The grid of n cells per axis over the box [lo, hi].
inline sdf_grid box_grid(const double (&lo)[3], const double (&hi)[3], int n, float iso = 0.0f) {
  sdf_grid g{};
  for (int c = 0; c < 3; ++c) {
    g.origin[c] = static_cast<float>(lo[c]);
    g.cell[c] = static_cast<float>((hi[c] - lo[c]) / n);
    g.n[c] = n;
  }
  g.iso = iso;
  return g;
}
// ---- measures (sdf_abi.h "Measures") ---------------------------------------------
// The integer rows of sdf_measure on the host, with the header's fp64
// conversions over the lattice coordinates origin + (i + 1/2) cell.  Row 0 is
// the whole solid; with owners, row 1 + k the samples primitive k owns.
struct Moments {
  double m0, m1[3], m2[3][3];   // sums of w, w i_c, w i_c i_d
};
struct Measure {
  std::vector<int64_t> rows;    // 16 per row: one row, or 17 with owners
  int64_t counts[4];            // bricks evaluated, in closed form, in all, 0
  double origin[3], cell[3];
  int32_t n[3];

  bool owners() const { return rows.size() == size_t(SDF_MEASURE_ROWS) * SDF_MEASURE_SLOTS; }
  double cell_volume() const { return cell[0] * cell[1] * cell[2]; }
  static void add_row(Moments& m, const int64_t* r, double w) {
    static const int pair[6][2] = {{0, 0}, {1, 1}, {2, 2}, {0, 1}, {0, 2}, {1, 2}};
    m.m0 += w * double(r[0]);
    for (int c = 0; c < 3; ++c) m.m1[c] += w * double(r[1 + c]);
    for (int s = 0; s < 6; ++s) {
      m.m2[pair[s][0]][pair[s][1]] += w * double(r[4 + s]);
      if (pair[s][0] != pair[s][1]) m.m2[pair[s][1]][pair[s][0]] += w * double(r[4 + s]);
    }
  }
  // row 0's raw moments; with densities sum_k rho_k (N_k, S_k, Q_k) over the owner rows
  Moments moments(const std::vector<double>& densities = {}) const {
    Moments m{};
    if (densities.empty()) {
      add_row(m, rows.data(), 1.0);
      return m;
    }
    if (!owners() || densities.size() > size_t(SDF_MAX_PRIMS))
      throw Error(SDF_E_INVALID_ARG, "Measure: densities need the owner rows");
    for (size_t k = 0; k < densities.size(); ++k)
      add_row(m, rows.data() + (1 + k) * SDF_MEASURE_SLOTS, densities[k]);
    return m;
  }
  double volume() const { return double(rows[0]) * cell_volume(); }
  double mass(const std::vector<double>& densities) const {
    return moments(densities).m0 * cell_volume();
  }
  void centroid(double (&out)[3], const std::vector<double>& densities = {}) const {
    const Moments m = moments(densities);
    for (int c = 0; c < 3; ++c) out[c] = origin[c] + (m.m1[c] / m.m0 + 0.5) * cell[c];
  }
  // (every helper evaluates in the order of sdf3d_amd/measure.py, operation for
  // operation, so the two give the same fp64 bits)
  void covariance(double (&out)[3][3], const std::vector<double>& densities = {}) const {
    const Moments m = moments(densities);
    for (int c = 0; c < 3; ++c)
      for (int d = 0; d < 3; ++d)
        out[c][d] = (m.m2[c][d] / m.m0 - (m.m1[c] / m.m0) * (m.m1[d] / m.m0)) * (cell[c] * cell[d]) +
                    (c == d ? cell[c] * cell[c] / 12.0 : 0.0);
  }
  // about the centroid: mass (tr(C) Id - C), the mass density * volume or mass(densities)
  void inertia(double (&out)[3][3], double density = 1.0,
               const std::vector<double>& densities = {}) const {
    double cv[3][3];
    covariance(cv, densities);
    const double ms = densities.empty() ? density * volume() : mass(densities);
    const double tr = cv[0][0] + cv[1][1] + cv[2][2];
    for (int c = 0; c < 3; ++c)
      for (int d = 0; d < 3; ++d) out[c][d] = ms * ((c == d ? tr : 0.0) - cv[c][d]);
  }
  // the cells row 0 occupies; false for an empty set
  bool bounds(double (&lo)[3], double (&hi)[3]) const {
    if (rows[0] == 0) return false;
    for (int c = 0; c < 3; ++c) {
      lo[c] = origin[c] + double(rows[10 + c]) * cell[c];
      hi[c] = origin[c] + double(rows[13 + c] + 1) * cell[c];
    }
    return true;
  }
  // the measure whose row 0 combines the owner rows of `prims`
  Measure select(const std::vector<int>& prims) const {
    if (!owners()) throw Error(SDF_E_INVALID_ARG, "Measure: select needs the owner rows");
    Measure r = *this;
    r.rows.assign(SDF_MEASURE_SLOTS, 0);
    for (int c = 0; c < 3; ++c) {
      r.rows[10 + c] = n[c];
      r.rows[13 + c] = -1;
    }
    std::vector<bool> seen(SDF_MAX_PRIMS, false);
    for (int k : prims) {
      if (k < 0 || k >= SDF_MAX_PRIMS) throw Error(SDF_E_INVALID_ARG, "Measure: no such primitive");
      if (seen[k]) continue;
      seen[k] = true;
      const int64_t* q = rows.data() + (1 + k) * SDF_MEASURE_SLOTS;
      for (int j = 0; j < 10; ++j) r.rows[j] += q[j];
      for (int j = 10; j < 13; ++j) r.rows[j] = std::min(r.rows[j], q[j]);
      for (int j = 13; j < 16; ++j) r.rows[j] = std::max(r.rows[j], q[j]);
    }
    return r;
  }
};
// sdf_measure of the frame's scene on `grid`, and the copies back.  Blocking.
inline Measure measure(const Frame& f, const sdf_grid& grid, bool owners = false,
                       hipStream_t stream = nullptr) {
  check_abi();
  const int32_t flags = owners ? SDF_MEASURE_OWNERS : 0;
  check(sdf_validate_measure(&f.scene, &f.params, &grid, flags), "sdf_validate_measure");
  const int64_t bytes = sdf_measure_workspace_bytes(&grid, flags);
  if (bytes < 0) check(static_cast<int>(bytes), "sdf_measure_workspace_bytes");
  Measure m{};
  const size_t nrows = owners ? SDF_MEASURE_ROWS : 1, out_bytes = nrows * SDF_MEASURE_SLOTS * 8;
  m.rows.resize(nrows * SDF_MEASURE_SLOTS);
  for (int c = 0; c < 3; ++c) {
    m.origin[c] = grid.origin[c];
    m.cell[c] = grid.cell[c];
    m.n[c] = grid.n[c];
  }
  char *ws = nullptr, *out = nullptr;   // out: moments | counts
  int rc = SDF_OK;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&ws), size_t(bytes));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&out), out_bytes + 32);
  if (e == hipSuccess) {
    rc = sdf_measure(&f.scene, &f.params, &grid, flags, ws, bytes, reinterpret_cast<int64_t*>(out),
                     reinterpret_cast<int64_t*>(out + out_bytes), stream);
    if (rc == SDF_OK) e = hipStreamSynchronize(stream);
    if (rc == SDF_OK && e == hipSuccess)
      e = hipMemcpy(m.rows.data(), out, out_bytes, hipMemcpyDeviceToHost);
    if (rc == SDF_OK && e == hipSuccess)
      e = hipMemcpy(m.counts, out + out_bytes, 32, hipMemcpyDeviceToHost);
  }
  (void)hipFree(out);
  (void)hipFree(ws);
  check(rc, "sdf_measure");
  check_hip(e, "measure");
  return m;
}

// A Wavefront OBJ file of the mesh: 1-based indices, `vn` lines when the mesh
// has normals (sdf3d_amd/meshio.py reads it back).  `colors` (4 floats per
// vertex, as bake returns them; empty: none): every `v` line carries r g b
// behind the position.
inline void write_obj(const std::string& path, const Mesh& m,
                      const std::vector<float>& colors = {}) {
  FILE* fp = std::fopen(path.c_str(), "w");
  if (!fp) throw Error(SDF_E_INVALID_ARG, "cannot open " + path);
  const size_t nv = m.verts.size() / 3, nt = m.tris.size() / 3;
  const bool vn = m.normals.size() == m.verts.size() && nv > 0;
  const bool vc = colors.size() == 4 * nv && nv > 0;
  std::fprintf(fp, "# %zu vertices, %zu triangles\n", nv, nt);
  for (size_t i = 0; i < nv; ++i) {
    std::fprintf(fp, "v %.9g %.9g %.9g", m.verts[3 * i], m.verts[3 * i + 1], m.verts[3 * i + 2]);
    if (vc)
      std::fprintf(fp, " %.9g %.9g %.9g", colors[4 * i], colors[4 * i + 1], colors[4 * i + 2]);
    std::fputc('\n', fp);
  }
  if (vn)
    for (size_t i = 0; i < nv; ++i)
      std::fprintf(fp, "vn %.9g %.9g %.9g\n", m.normals[3 * i], m.normals[3 * i + 1],
                   m.normals[3 * i + 2]);
  for (size_t i = 0; i < nt; ++i) {
    const int a = m.tris[3 * i] + 1, b = m.tris[3 * i + 1] + 1, c = m.tris[3 * i + 2] + 1;
    if (vn) std::fprintf(fp, "f %d//%d %d//%d %d//%d\n", a, a, b, b, c, c);
    else std::fprintf(fp, "f %d %d %d\n", a, b, c);
  }
  std::fclose(fp);
}

// ---- shading at caller-supplied points (sdf_abi.h "Points") ---------------------
// Lights, shadows, occlusion and materials of the frame's scene at n points of
// the caller's own, without a primary march: `points` (device, n x 3 packed
// floats), `normals` (the same, used as given, or null: evaluated at the point),
// `eye` (3 floats, or null: no specular term), `lift` (the points move that far
// along their normals first).  `out`: device buffers, null for what is not
// wanted (sdf_point_shade).  An empty `materials` gives every primitive
// f.material, an empty `lights` the frame's one.  A wave shades 64 consecutive
// points.  Asynchronous on `stream`.
inline void shade_points(const Frame& f, const std::vector<sdf_light>& lights, int32_t light_flags,
                         const std::vector<sdf_material>& materials, const float* points,
                         const float* normals, int64_t n, const float* eye, float lift,
                         const sdf_point_shade& out, hipStream_t stream = nullptr) {
  const std::vector<sdf_material> m = f.table(materials);
  const std::vector<sdf_light> one(1, f.light);
  const std::vector<sdf_light>& l = lights.empty() ? one : lights;
  sdf_points p{};
  p.points = points;
  p.normals = normals;
  p.n = n;
  p.lift = lift;
  if (eye) {
    p.flags = SDF_POINTS_EYE;
    for (int c = 0; c < 3; ++c) p.eye[c] = eye[c];
  }
  check(sdf_shade_points(&f.scene, l.data(), static_cast<int32_t>(l.size()), light_flags, m.data(),
                         static_cast<int32_t>(m.size()), &f.params, &p, &out, stream),
        "sdf_shade_points");
}
// Vertex colours of a mesh extracted with `grid` (4 floats per vertex, alpha 1):
// shade_points at the vertices with the mesh's normals when it has them, lifted
// by the length of the cell diagonal (a surface-nets vertex lies within half a
// diagonal of the surface) unless `lift` >= 0 says otherwise.  Blocking.
inline std::vector<float> bake(const Frame& f, const Mesh& m, const sdf_grid& grid,
                               const std::vector<sdf_light>& lights = {}, int32_t light_flags = 0,
                               const std::vector<sdf_material>& materials = {},
                               const float* eye = nullptr, float lift = -1.0f,
                               hipStream_t stream = nullptr) {
  check_abi();
  const size_t nv = m.verts.size() / 3;
  std::vector<float> colors(4 * nv);
  if (nv == 0) return colors;
  if (lift < 0.0f) {
    double d2 = 0.0;
    for (int c = 0; c < 3; ++c) d2 += double(grid.cell[c]) * double(grid.cell[c]);
    lift = static_cast<float>(std::sqrt(d2));
  }
  const bool vn = m.normals.size() == m.verts.size();
  // colours | verts | normals: the colours first, 16-byte aligned as rgba must be
  const size_t oc = 0, ov = nv * 16, on = ov + nv * 12, end = on + (vn ? nv * 12 : 0);
  char* buf = nullptr;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&buf), end);
  int rc = SDF_OK;
  try {
    if (e == hipSuccess)
      e = hipMemcpyAsync(buf + ov, m.verts.data(), nv * 12, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && vn)
      e = hipMemcpyAsync(buf + on, m.normals.data(), nv * 12, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) {
      sdf_point_shade out{};
      out.rgba = reinterpret_cast<float*>(buf + oc);
      shade_points(f, lights, light_flags, materials, reinterpret_cast<const float*>(buf + ov),
                   vn ? reinterpret_cast<const float*>(buf + on) : nullptr,
                   static_cast<int64_t>(nv), eye, lift, out, stream);
      e = hipMemcpyAsync(colors.data(), buf + oc, nv * 16, hipMemcpyDeviceToHost, stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
  } catch (const Error& err) {
    rc = err.code;
  }
  (void)hipFree(buf);
  check(rc, "sdf_shade_points");
  check_hip(e, "bake");
  return colors;
}
// A colour component as a byte by the RGBA8 rule of sdf_abi.h: trunc(min(max(c,
// 0), 1) * 255 + 0.5) in fp32, NaN -> 0.
inline unsigned char color_u8(float c) {
  if (!(c == c)) return 0;
  const float x = c < 0.0f ? 0.0f : (c > 1.0f ? 1.0f : c);
  const volatile float y = x * 255.0f;   // rounded before the sum: no fusion
  return static_cast<unsigned char>(y + 0.5f);
}
// A binary little-endian PLY file of the mesh: float x y z, float nx ny nz when
// the mesh has normals, uchar red green blue when `colors` (4 floats per vertex)
// has one per vertex, then the triangles (sdf3d_amd/meshio.py reads it back).
inline void write_ply(const std::string& path, const Mesh& m,
                      const std::vector<float>& colors = {}) {
  FILE* fp = std::fopen(path.c_str(), "wb");
  if (!fp) throw Error(SDF_E_INVALID_ARG, "cannot open " + path);
  const size_t nv = m.verts.size() / 3, nt = m.tris.size() / 3;
  const bool vn = m.normals.size() == m.verts.size() && nv > 0;
  const bool vc = colors.size() == 4 * nv && nv > 0;
  std::fprintf(fp, "ply\nformat binary_little_endian 1.0\nelement vertex %zu\n"
                   "property float x\nproperty float y\nproperty float z\n", nv);
  if (vn) std::fprintf(fp, "property float nx\nproperty float ny\nproperty float nz\n");
  if (vc) std::fprintf(fp, "property uchar red\nproperty uchar green\nproperty uchar blue\n");
  std::fprintf(fp, "element face %zu\nproperty list uchar int vertex_indices\nend_header\n", nt);
  for (size_t i = 0; i < nv; ++i) {
    std::fwrite(&m.verts[3 * i], 4, 3, fp);
    if (vn) std::fwrite(&m.normals[3 * i], 4, 3, fp);
    if (vc) {
      const unsigned char c[3] = {color_u8(colors[4 * i]), color_u8(colors[4 * i + 1]),
                                  color_u8(colors[4 * i + 2])};
      std::fwrite(c, 1, 3, fp);
    }
  }
  for (size_t i = 0; i < nt; ++i) {
    const unsigned char three = 3;
    std::fwrite(&three, 1, 1, fp);
    std::fwrite(&m.tris[3 * i], 4, 3, fp);
  }
  std::fclose(fp);
}

// ---- multi-device frames (sdf_comm_* / sdf_driver_*) ------------------------

// One RCCL communicator over `world` processes (one per GPU), created from a
// unique id rank 0 makes; the caller moves the id between processes.
class Comm {
 public:
  using Id = std::vector<unsigned char>;
  static Id unique_id(const std::string& rccl_path = "") {
    check_abi();
    Id id(SDF_COMM_ID_BYTES);
    check(sdf_comm_unique_id(rccl_path.empty() ? nullptr : rccl_path.c_str(), id.data()),
          "sdf_comm_unique_id");
    return id;
  }
  // Blocks until every rank has joined, at most timeout_ms (then throws
  // SDF_E_TIMEOUT: a peer that failed, or an id that is not this launch's).
  Comm(const Id& id, int world, int rank, const std::string& rccl_path = "",
       int timeout_ms = 120000) {
    check_abi();
    check(sdf_comm_create(rccl_path.empty() ? nullptr : rccl_path.c_str(), id.data(), world, rank,
                          timeout_ms, &c_),
          "sdf_comm_create");
  }
  ~Comm() { if (c_) (void)sdf_comm_destroy(c_); }
  Comm(const Comm&) = delete;
  Comm& operator=(const Comm&) = delete;
  sdf_comm* get() const { return c_; }

 private:
  sdf_comm* c_ = nullptr;
};

// Moves communicator ids through a directory every rank can see (a node's
// local disk or /dev/shm): rank 0 writes `name` atomically (write, then
// rename), the others wait for it.  Pure-C++ launches (no MPI, no Python)
// use this; a Python host uses torch.distributed (sdf3d_amd/driver.py).
//
// A file left by an earlier launch that died before rank 0 removed it must
// not be taken for this launch's.  So the file carries a launch tag (the
// launcher's MASTER_ADDR/MASTER_PORT, TORCHELASTIC_RUN_ID and
// TORCHELASTIC_RESTART_COUNT, plus SDF3D_LAUNCH_NONCE when the launcher
// sets one) that peers compare with their own, and peers ignore a file
// written before their own first call here, less `skew_s` (ranks of one
// launch start within seconds of each other).  An id that still slips
// through cannot hang anyone: Comm's join gives up after its timeout.
inline std::string launch_tag() {
  std::string t;
  for (const char* k : {"MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID",
                        "TORCHELASTIC_RESTART_COUNT", "SDF3D_LAUNCH_NONCE"}) {
    const char* v = std::getenv(k);
    t += std::string(k) + "=" + (v ? v : "") + ";";
  }
  return t;
}

inline Comm::Id exchange_id(const std::string& dir, const std::string& name, int rank,
                            const std::string& rccl_path = "", double timeout_s = 120.0,
                            double skew_s = 30.0) {
  static const auto first_call = std::chrono::system_clock::now();
  const std::string path = dir + "/" + name;
  const std::string tag = launch_tag();
  if (rank == 0) {
    Comm::Id id = Comm::unique_id(rccl_path);
    const std::string tmp = path + ".tmp";
    const uint32_t n = static_cast<uint32_t>(tag.size());
    FILE* fp = std::fopen(tmp.c_str(), "wb");
    if (!fp || std::fwrite(&n, sizeof(n), 1, fp) != 1 ||
        std::fwrite(tag.data(), 1, n, fp) != n ||
        std::fwrite(id.data(), 1, id.size(), fp) != id.size() || std::fclose(fp) != 0 ||
        std::rename(tmp.c_str(), path.c_str()) != 0)
      throw std::runtime_error("cannot write " + path);
    return id;
  }
  const auto not_before = first_call - std::chrono::milliseconds(long(skew_s * 1e3));
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    struct stat sb;
    if (stat(path.c_str(), &sb) == 0 &&
        std::chrono::system_clock::from_time_t(sb.st_mtime) >= not_before) {
      if (FILE* fp = std::fopen(path.c_str(), "rb")) {
        uint32_t n = 0;
        std::string got;
        Comm::Id id(SDF_COMM_ID_BYTES);
        bool ok = std::fread(&n, sizeof(n), 1, fp) == 1 && n < (1u << 16);
        if (ok) {
          got.resize(n);
          ok = std::fread(&got[0], 1, n, fp) == n &&
               std::fread(id.data(), 1, id.size(), fp) == id.size();
        }
        std::fclose(fp);
        if (ok && got == tag) return id;
      }
    }
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s)
      throw std::runtime_error("timed out waiting for " + path + " of this launch");
    std::this_thread::sleep_for(std::chrono::milliseconds(5));
  }
}

// The native frame loop across the node (include/sdf_abi.h sdf_driver_*):
// every rank steps every frame; rank 0 holds the assembled frames.  The
// reference's `while (!gl->closed()) { ... gl->plot(sh, proj_mode); }`
// (main.cpp:87-98) becomes `while (...) { drv.set_camera(...); drv.step(); }`.
class FrameDriver {
 public:
  FrameDriver(const Frame& f, const sdf_driver_config& cfg, Comm* lengths = nullptr,
              Comm* data = nullptr)
      : w_(f.params.width), h_(f.params.height), format_(f.params.output_format) {
    check_abi();
    check(sdf_driver_create(&f.scene, &f.camera, &f.light, &f.material, &f.params, &cfg,
                            lengths ? lengths->get() : nullptr, data ? data->get() : nullptr, &d_),
          "sdf_driver_create");
  }
  ~FrameDriver() { if (d_) (void)sdf_driver_destroy(d_); }
  FrameDriver(const FrameDriver&) = delete;
  FrameDriver& operator=(const FrameDriver&) = delete;

  void set_camera(const sdf_camera& c) { check(sdf_driver_set_camera(d_, &c), "sdf_driver_set_camera"); }
  int64_t step() {
    int64_t i = -1;
    check(sdf_driver_step(d_, &i), "sdf_driver_step");
    return i;
  }
  void drain() { check(sdf_driver_drain(d_), "sdf_driver_drain"); }
  // Rank 0: blocking copy of frame i (one of the last nbuf, shipped).
  std::vector<float> download(int64_t i) const {
    if (format_ != SDF_FORMAT_RGBA32F) throw Error(SDF_E_UNSUPPORTED, "download: not RGBA32F");
    std::vector<float> out(size_t(w_) * h_ * 4);
    void* src = nullptr;
    check(sdf_driver_frame(d_, i, &src), "sdf_driver_frame");
    check_hip(hipDeviceSynchronize(), "hipDeviceSynchronize");
    check_hip(hipMemcpy(out.data(), src, out.size() * sizeof(float), hipMemcpyDeviceToHost),
              "hipMemcpy");
    return out;
  }
  // Host seconds of the driver's own calls per frame, waits excluded.
  double host_us_per_frame() const {
    double v[3] = {0, 0, 0};
    check(sdf_driver_stats(d_, v, 3), "sdf_driver_stats");
    return v[0] > 0 ? (v[1] - v[2]) / v[0] * 1e6 : 0.0;
  }

 private:
  int w_, h_, format_;
  sdf_driver* d_ = nullptr;
};

// One RGBA32F frame across several devices of this process (sdf_render_multi):
// devices[0] holds `rgba` and `stream`; the others render TILES streams the
// root decodes through peer-mapped memory.  Successive calls on one stream.
inline void render_multi(const Frame& f, const std::vector<int>& devices, float* rgba,
                         hipStream_t stream, int share_root = 0, int share_peer = 0) {
  check_abi();
  std::vector<int32_t> d(devices.begin(), devices.end());
  check(sdf_render_multi(&f.scene, &f.camera, &f.light, &f.material, &f.params,
                         static_cast<int32_t>(d.size()), d.data(), share_root, share_peer, rgba,
                         stream),
        "sdf_render_multi");
}

// A camera path known in advance (sdf_render_frames): frame i of `f`'s scene
// seen through cameras[i] into rgba[i] (steps[i] when `steps` is non-empty),
// by the persistent frame-sequence kernel; the pixels of one sdf_render per
// camera.  Asynchronous on `stream`.
inline void render_frames(const Frame& f, const std::vector<sdf_camera>& cameras,
                          const std::vector<void*>& rgba, hipStream_t stream,
                          const std::vector<int32_t*>& steps = {}) {
  check_abi();
  if (rgba.size() != cameras.size() || (!steps.empty() && steps.size() != cameras.size()))
    throw Error(SDF_E_INVALID_ARG, "render_frames: one output per camera");
  check(sdf_render_frames(&f.scene, cameras.data(), static_cast<int32_t>(cameras.size()),
                          &f.light, &f.material, &f.params, rgba.data(),
                          steps.empty() ? nullptr : steps.data(), stream),
        "sdf_render_frames");
}

// Binary PPM of an RGBA float framebuffer, clamped and quantised to 8 bits
// (what the reference's window would show), flipped to top-down row order.
inline void write_ppm(const std::string& path, const std::vector<float>& rgba, int w, int h) {
  FILE* fp = std::fopen(path.c_str(), "wb");
  if (!fp) throw std::runtime_error("cannot open " + path);
  std::fprintf(fp, "P6\n%d %d\n255\n", w, h);
  std::vector<unsigned char> row(size_t(w) * 3);
  for (int y = h - 1; y >= 0; --y) {
    for (int x = 0; x < w; ++x)
      for (int c = 0; c < 3; ++c) {
        float v = rgba[(size_t(y) * w + x) * 4 + c];
        v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
        row[size_t(x) * 3 + c] = static_cast<unsigned char>(std::lround(v * 255.0f));
      }
    std::fwrite(row.data(), 1, row.size(), fp);
  }
  std::fclose(fp);
}

}  // namespace sdf
