// sdf_main.cpp -- headless counterpart of the reference host program
// (/root/reference/Code/src/main.cpp): create the renderer once, loop over
// frames (the reference's `while(!gl->closed())` with arcball input, :87-98,
// becomes an orbit sequence), time each frame (the reference's unreported
// cl->get_tic()/get_toc(), :89/:97) and clean up.  The last frame is written
// as a PPM instead of being presented in a window (:95-96).
//
//   sdf_main [--palette] [--reflect B[,strength]] [--sky [--no-sun]] [--fog START,END[,r,g,b]]
//            [--pick X,Y] [--projection pinhole|equirect]
//            [--mesh FILE.obj|FILE.ply --grid x0,y0,z0,x1,y1,z1,N [--mesh-colors]
//             [--mesh-sharp [R,K]]]
//            [--measure x0,y0,z0,x1,y1,z1,N [--density d0,d1,...]]
//            [width height frames out.ppm scene [samples [lights]]]
//     scene: ref | csg8 | bulb; samples: 1 (default), 2 or 4 sub-samples per
//     axis, resolved in the render kernel (single-GPU path only: the frame
//     driver refuses supersampling)
//     lights: "x,y,z[,r,g,b];..." -- up to SDF_MAX_LIGHTS point lights that
//     light the frame together (sdf_render_lights; single-GPU path only).  The
//     first carries the reference's ambient term, the others none; a light
//     with r,g,b turns SDF_LIGHTS_COLOR on (lights without get white).  The
//     default is the reference's one light.
//     --palette (anywhere on the line): a material per primitive from
//     sdf::palette, blended along the CSG fold (sdf_render_materials;
//     single-GPU path only); a Mandelbulb gets the palette's first entry
//     --reflect B[,strength] (anywhere on the line): B = 0 .. SDF_MAX_BOUNCES
//     mirror bounces per pixel, every surface's ref times strength (default
//     1) weighting what it reflects (sdf_render_reflect; single-GPU path
//     only); without --palette every primitive has the reference's material
//     --sky (anywhere on the line): rays that leave the scene show sdf::sky(),
//     the default sky with its sun, instead of shading the far point; with
//     --no-sun (anywhere on the line) the sky without the sun's glow
//     --fog START,END[,r,g,b] (anywhere on the line): linear distance fog from
//     START to END in the sky's horizon colour, or in r,g,b (both:
//     sdf_render_env, single-GPU path only; without --reflect no bounce)
//     --pick X,Y (anywhere on the line): after the last frame, what lies under
//     its pixel X,Y (row 0 = bottom) through that frame's camera, one ray per
//     pixel (sdf_trace_camera; single-GPU path only), printed as
//     "pick X,Y: t steps prim nx ny nz" -- prim is the index of the primitive
//     that owns the hit, -1 when the ray leaves the scene
//     --projection pinhole|equirect (anywhere on the line): the frame shaded
//     from a list of rays (sdf_render_rays; single-GPU path only, one sample
//     per pixel).  pinhole: the render's own rays from sdf_camera_rays, used
//     as given (SDF_RAYS_UNIT) -- the frame without the option, bit for bit in
//     exact precision.  equirect: a full panorama from the camera's place,
//     longitude across and latitude up, its directions built on the host and
//     normalised by the kernel
//     --mesh FILE.obj|FILE.ply --grid x0,y0,z0,x1,y1,z1,N (anywhere on the line): after
//     the last frame, the scene's surface inside the box from (x0,y0,z0) to
//     (x1,y1,z1), N cells per axis, as a triangle mesh with normals in a
//     Wavefront OBJ file (sdf::extract_mesh: sdf_mesh_count and sdf_mesh_emit;
//     single-GPU path only); a FILE ending in .ply is written as binary PLY.
//     With --mesh-colors every vertex carries its baked colour (sdf::bake:
//     sdf_shade_points at the vertices, lifted by one cell diagonal, under the
//     frame's lights and, with --palette, its materials; no specular term, which
//     would depend on the viewer).  With --mesh-sharp the vertices lie on the
//     scene's edges and corners instead of chamfering them (sdf_mesh_emit_sharp:
//     R refinement steps per crossing and K steps of the fit, 4,16 when not
//     given; not for a Mandelbulb).  --palette stays the switch it is above: it
//     takes no count, the palette has one entry per primitive
//     --measure x0,y0,z0,x1,y1,z1,N [--density d0,d1,...] (anywhere on the line):
//     after the last frame, one JSON line with the volume, mass, centroid, inertia
//     tensor about the centroid and bounds of the solid inside the box, N cells
//     per axis (sdf::measure: sdf_measure; single-GPU path only), and the bricks
//     evaluated, taken in closed form and in all.  --density gives a density per
//     primitive (in list order; a ground plane gets 0 to be left out): mass,
//     centroid and inertia are then the weighted ones; without it the density is 1
//
// Multi-GPU: launched once per GPU by any launcher that sets RANK,
// WORLD_SIZE and LOCAL_RANK (e.g. `torchrun --nproc-per-node 8 --no-python
// sdf_main 3840 2160 200 out.ppm csg8`), or with SDF3D_DRIVER=1 on one GPU,
// it runs the native frame driver (sdf_driver_*): every rank renders its row
// blocks of every frame and rank 0 assembles them over RCCL.  The two RCCL
// unique ids travel through files in SDF3D_ID_DIR (default /tmp) named by
// SDF3D_RUN_ID (default: torchrun's TORCHELASTIC_RUN_ID); SDF3D_RCCL names
// the librccl to load (default librccl.so.1); SDF3D_ROOT_AS_PEER=1 makes
// rank 0 ship its rows to itself (the multi-rank sequence on one GPU).
//
// Navigation: by default frame i orbits the camera by 360 i / frames degrees;
// SDF3D_NAV=arcball drives V_mat from sdf::Arcball (the reference's mouse and
// gamepad navigation, main.cpp:37-45, :93-94) fed with a scripted input
// sequence (nav_input: orbit drag, pan drag, release, gamepad sticks), and
//   sdf_main --views N
// prints the first N V_mats of that sequence (no GPU work; the tests compare
// them with sdf3d_amd.camera.Arcball fed the same script).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../include/sdf3d.hpp"

namespace {

std::string env(const char* name, const char* dflt) {
  const char* v = std::getenv(name);
  return v && *v ? v : dflt;
}

// The scripted navigation input of frame i (period 90 frames at 60 Hz),
// restated in tests/test_camera.py nav_input.
void nav_input(sdf::Arcball& a, int i) {
  const double dt = 1.0 / 60.0;
  const int ph = i % 90;
  if (ph < 30) a.mouse(dt, 0.004, 0.0015, true, false);          // orbit drag
  else if (ph < 45) a.mouse(dt, -0.002, 0.001, false, true);     // pan drag
  else if (ph < 60) a.mouse(dt, 0.0, 0.0, false, false);         // released: decay
  else if (ph < 80) a.gamepad(dt, 0.8, -0.5, 0.2, 0.35);        // sticks (rx inside the deadzone)
  else a.gamepad(dt, 0.1, 0.0, 0.0, 0.0);                        // sticks released
}

// V_mat of frame i under SDF3D_NAV (see the header comment).
struct Navigator {
  bool arcball = env("SDF3D_NAV", "orbit") == "arcball";
  sdf::Arcball ball;
  int next = 0;
  void frame(sdf::Frame& f, int i, int frames) {
    if (!arcball) {
      f.orbit(360.0f * i / frames, 0.0f);
      return;
    }
    while (next <= i) nav_input(ball, next++);
    ball.apply(f);
  }
};

// argv[7]: "x,y,z[,r,g,b];..." (see the header comment)
bool parse_lights(const std::string& text, const sdf_light& first, std::vector<sdf_light>& lights,
                  int32_t& flags) {
  size_t at = 0;
  while (at < text.size()) {
    size_t end = text.find(';', at);
    if (end == std::string::npos) end = text.size();
    const std::string item = text.substr(at, end - at);
    at = end + 1;
    if (item.empty()) continue;
    float v[6];
    const int n = std::sscanf(item.c_str(), "%f,%f,%f,%f,%f,%f", &v[0], &v[1], &v[2], &v[3], &v[4],
                              &v[5]);
    if (n != 3 && n != 6) return false;
    sdf_light l = first;
    l.ambient = lights.empty() ? first.ambient : 0.0f;
    for (int c = 0; c < 3; ++c) {
      l.pos[c] = v[c];
      l.color[c] = n == 6 ? v[3 + c] : 1.0f;
    }
    if (n == 6) flags |= SDF_LIGHTS_COLOR;
    lights.push_back(l);
  }
  return !lights.empty() && lights.size() <= SDF_MAX_LIGHTS;
}

int run_driver(sdf::Frame f, int frames, const std::string& out) {
  const int rank = std::atoi(env("RANK", "0").c_str());
  const int world = std::atoi(env("WORLD_SIZE", "1").c_str());
  const int local = std::atoi(env("LOCAL_RANK", "0").c_str());
  const bool peer_root = env("SDF3D_ROOT_AS_PEER", "0") == "1";
  sdf::check_hip(hipSetDevice(local), "hipSetDevice");
  const std::string rccl = env("SDF3D_RCCL", "librccl.so.1");
  const std::string dir = env("SDF3D_ID_DIR", "/tmp");
  const std::string run = env("SDF3D_RUN_ID", env("TORCHELASTIC_RUN_ID", "default").c_str());
  std::unique_ptr<sdf::Comm> lengths, data;
  if (world > 1 || peer_root) {
    const std::string a = "sdf3d_" + run + "_lengths.id", b = "sdf3d_" + run + "_data.id";
    lengths.reset(new sdf::Comm(sdf::exchange_id(dir, a, rank, rccl), world, rank, rccl));
    data.reset(new sdf::Comm(sdf::exchange_id(dir, b, rank, rccl), world, rank, rccl));
    if (rank == 0) {  // every rank has joined both communicators: the files are spent
      std::remove((dir + "/" + a).c_str());
      std::remove((dir + "/" + b).c_str());
    }
  }
  // shares: SDF3D_SHARES="a:b", else what the cost model of bench.py picks
  // for this world size (sdf3d_amd/multigpu.py choose_shares)
  static const int kShares[9][2] = {{1, 1}, {1, 1}, {1, 1}, {1, 1}, {3, 4},
                                    {3, 4}, {1, 2}, {1, 2}, {1, 7}};
  int share_root = kShares[world < 9 ? world : 8][0], share_peer = kShares[world < 9 ? world : 8][1];
  if (std::sscanf(env("SDF3D_SHARES", "").c_str(), "%d:%d", &share_root, &share_peer) != 2) {
    share_root = kShares[world < 9 ? world : 8][0];
    share_peer = kShares[world < 9 ? world : 8][1];
  }
  // N > 1: frames shipped two at a time (one length all-gather and one
  // send/recv group per pair), 4 buffer sets, a pair gathered 2 frames after
  // its last render
  const bool ship = world > 1 || peer_root;
  sdf_driver_config cfg = {rank, world, share_root, share_peer, ship ? 4 : 3, ship ? 2 : 1,
                           peer_root ? SDF_DRIVER_ROOT_AS_PEER : 0, 60000, ship ? 2 : 1};
  f.params.output_format = SDF_FORMAT_RGBA32F;
  sdf::FrameDriver drv(f, cfg, lengths.get(), data.get());
  int64_t last = -1;
  for (int i = 0; i < 5; ++i) last = drv.step();  // warm-up
  drv.drain();
  Navigator nav;
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < frames; ++i) {
    nav.frame(f, i, frames);                        // the arcball's V_mat (main.cpp:93-94)
    drv.set_camera(f.camera);
    last = drv.step();
  }
  drv.drain();
  const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (rank == 0) {
    std::printf("rank 0 of %d: %d frames %dx%d in %.3f ms: %.1f fps, %.1f Mpixels/s "
                "(driver host %.1f us/frame)\n",
                world, frames, f.params.width, f.params.height, s * 1e3, frames / s,
                double(f.params.width) * f.params.height * frames / s / 1e6,
                drv.host_us_per_frame());
    sdf::write_ppm(out, drv.download(last), f.params.width, f.params.height);
    std::printf("wrote %s\n", out.c_str());
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 2 && std::string(argv[1]) == "--views") {
    sdf::Arcball ball;
    float v[16];
    for (int i = 0; i < std::atoi(argv[2]); ++i) {
      nav_input(ball, i);
      ball.view(v);
      for (int k = 0; k < 16; ++k) {
        uint32_t u;
        std::memcpy(&u, &v[k], 4);
        std::printf("%08x%c", u, k == 15 ? '\n' : ' ');
      }
    }
    return 0;
  }
  // --palette and --reflect may stand anywhere: take them out of the
  // positional arguments
  bool use_palette = false, use_reflect = false, use_env = false, use_pick = false;
  bool no_sun = false;
  std::string projection, mesh_path;
  double box[6] = {0, 0, 0, 0, 0, 0};
  int mesh_n = 0;
  bool mesh_colors = false;
  sdf_mesh_sharp mesh_sharp = {0, 0, 0, 0};   // --mesh-sharp [R,K]
  bool use_mesh_sharp = false;
  double measure_box[6] = {0, 0, 0, 0, 0, 0};   // --measure x0,y0,z0,x1,y1,z1,N
  int measure_n = 0;
  std::vector<double> densities;                // --density d0,d1,...
  int pick_x = 0, pick_y = 0;
  sdf_reflect reflect = {0, 1.0f, -1, 0};
  sdf_environment environment = sdf::sky(0);
  {
    int n = 1;
    for (int i = 1; i < argc; ++i) {
      if (std::string(argv[i]) == "--palette") {
        use_palette = true;
      } else if (std::string(argv[i]) == "--reflect") {
        char* end = nullptr;
        const char* v = i + 1 < argc ? argv[++i] : "";
        reflect.bounces = static_cast<int32_t>(std::strtol(v, &end, 10));
        use_reflect = end != v;
        if (use_reflect && *end == ',') {
          const char* s = end + 1;
          reflect.strength = std::strtof(s, &end);
          use_reflect = end != s;
        }
        if (!use_reflect || *end != '\0') {
          std::fprintf(stderr, "sdf_main: --reflect B[,strength]\n");
          return 1;
        }
      } else if (std::string(argv[i]) == "--pick") {
        char tail = 0;
        use_pick = i + 1 < argc &&
                   std::sscanf(argv[++i], "%d,%d%c", &pick_x, &pick_y, &tail) == 2;
        if (!use_pick) {
          std::fprintf(stderr, "sdf_main: --pick X,Y\n");
          return 1;
        }
      } else if (std::string(argv[i]) == "--mesh") {
        mesh_path = i + 1 < argc ? argv[++i] : "";
        if (mesh_path.empty()) {
          std::fprintf(stderr, "sdf_main: --mesh FILE.obj|FILE.ply\n");
          return 1;
        }
      } else if (std::string(argv[i]) == "--mesh-colors") {
        mesh_colors = true;
      } else if (std::string(argv[i]) == "--mesh-sharp") {
        use_mesh_sharp = true;
        mesh_sharp.refine = 4;
        mesh_sharp.iterations = 16;
        // R,K when the next word is two numbers; anything else is the next option
        int r = 0, k = 0;
        char tail = 0;
        if (i + 1 < argc && std::sscanf(argv[i + 1], "%d,%d%c", &r, &k, &tail) == 2) {
          mesh_sharp.refine = r;
          mesh_sharp.iterations = k;
          ++i;
        }
      } else if (std::string(argv[i]) == "--grid") {
        char tail = 0;
        if (!(i + 1 < argc && std::sscanf(argv[++i], "%lf,%lf,%lf,%lf,%lf,%lf,%d%c", &box[0], &box[1],
                                          &box[2], &box[3], &box[4], &box[5], &mesh_n, &tail) == 7 &&
              mesh_n >= 1)) {
          std::fprintf(stderr, "sdf_main: --grid x0,y0,z0,x1,y1,z1,N\n");
          return 1;
        }
      } else if (std::string(argv[i]) == "--measure") {
        char tail = 0;
        double* b = measure_box;
        if (!(i + 1 < argc && std::sscanf(argv[++i], "%lf,%lf,%lf,%lf,%lf,%lf,%d%c", &b[0], &b[1], &b[2],
                                          &b[3], &b[4], &b[5], &measure_n, &tail) == 7 &&
              measure_n >= 1)) {
          std::fprintf(stderr, "sdf_main: --measure x0,y0,z0,x1,y1,z1,N\n");
          return 1;
        }
      } else if (std::string(argv[i]) == "--density") {
        const char* p = i + 1 < argc ? argv[++i] : "";
        char* end = nullptr;
        for (;;) {
          const double d = std::strtod(p, &end);
          if (end == p) break;
          densities.push_back(d);
          if (*end != ',') break;
          p = end + 1;
        }
        if (densities.empty() || *end != '\0' || densities.size() > SDF_MAX_PRIMS) {
          std::fprintf(stderr, "sdf_main: --density d0,d1,... (at most %d)\n", SDF_MAX_PRIMS);
          return 1;
        }
      } else if (std::string(argv[i]) == "--projection") {
        projection = i + 1 < argc ? argv[++i] : "";
        if (projection != "pinhole" && projection != "equirect") {
          std::fprintf(stderr, "sdf_main: --projection pinhole|equirect\n");
          return 1;
        }
      } else if (std::string(argv[i]) == "--sky") {
        environment.flags |= SDF_ENV_SKY | SDF_ENV_SUN;
        use_env = true;
      } else if (std::string(argv[i]) == "--no-sun") {
        no_sun = true;
      } else if (std::string(argv[i]) == "--fog") {
        // 2 or 5 comma-separated numbers
        float v[5];
        int nv = 0;
        const char* p = i + 1 < argc ? argv[++i] : "";
        char* end = nullptr;
        bool ok = true;
        while (ok && nv < 5) {
          v[nv] = std::strtof(p, &end);
          ok = end != p;
          if (!ok) break;
          ++nv;
          if (*end != ',') break;
          p = end + 1;
        }
        if (!ok || *end != '\0' || (nv != 2 && nv != 5)) {
          std::fprintf(stderr, "sdf_main: --fog START,END[,r,g,b]\n");
          return 1;
        }
        environment = sdf::fog(environment, v[0], v[1], nv == 5 ? v + 2 : nullptr);
        use_env = true;
      } else {
        argv[n++] = argv[i];
      }
    }
    argc = n;
    if (mesh_path.empty() != (mesh_n == 0)) {
      std::fprintf(stderr, "sdf_main: --mesh FILE.obj|FILE.ply needs --grid x0,y0,z0,x1,y1,z1,N and vice versa\n");
      return 1;
    }
    if ((mesh_colors || use_mesh_sharp) && mesh_path.empty()) {
      std::fprintf(stderr, "sdf_main: --mesh-colors and --mesh-sharp need --mesh FILE --grid ...\n");
      return 1;
    }
    if (!densities.empty() && measure_n == 0) {
      std::fprintf(stderr, "sdf_main: --density needs --measure x0,y0,z0,x1,y1,z1,N\n");
      return 1;
    }
    if (no_sun) environment.flags &= ~SDF_ENV_SUN;
  }
  const int W = argc > 1 ? std::atoi(argv[1]) : 800;   // main.cpp:4 SX
  const int H = argc > 2 ? std::atoi(argv[2]) : 600;   // main.cpp:5 SY
  const int frames = argc > 3 ? std::atoi(argv[3]) : 8;
  const std::string out = argc > 4 ? argv[4] : "sdf_main.ppm";
  const std::string kind = argc > 5 ? argv[5] : "ref";
  const int samples = argc > 6 ? std::atoi(argv[6]) : 1;
  try {
    sdf::Frame f = sdf::Frame::reference(W, H);
    std::vector<sdf_light> lights;
    int32_t light_flags = 0;
    if (argc > 7 && !parse_lights(argv[7], f.light, lights, light_flags))
      throw sdf::Error(SDF_E_INVALID_ARG, "lights: \"x,y,z[,r,g,b];...\", at most 8");
    f.supersample(samples);
    if (kind == "csg8") {
      const int S = SDF_OP_SMOOTH_UNION;
      const float k = 0.1f;
      sdf::Scene s;
      s.plane(0, 1, 0, 0)
          .sphere(0, 0.4f, 0, 0.2f, S, k)
          .box(-0.7f, 0.15f, -0.3f, 0.15f, 0.15f, 0.15f, S, k)
          .torus(0.7f, 0.1f, -0.3f, 0.2f, 0.06f, S, k)
          .capsule(-0.35f, 0.1f, 0.4f, 0.05f, 0.45f, 0.3f, 0.07f, S, k)
          .cylinder(0.45f, 0.25f, 0.35f, 0.12f, 0.25f, S, k)
          .round_box(0, 0.12f, -0.8f, 0.5f, 0.12f, 0.1f, 0.04f, S, k)
          .sphere(0.25f, 0.55f, -0.15f, 0.12f, S, k);
      f.scene = s.raw();
      f.params.max_steps = 128;
      f.params.flags = SDF_FLAG_SHADOW | SDF_FLAG_AO;
      f.params.normal_mode = SDF_NORMAL_TETRA;
    } else if (kind == "bulb") {
      f.scene = sdf::Scene().mandelbulb(0, 0.3f, 0, 0.45f).raw();
      f.params.max_steps = 128;
      f.params.flags = SDF_FLAG_SHADOW | SDF_FLAG_AO;
      f.params.normal_mode = SDF_NORMAL_TETRA;
    }
    // EXACT (the default): the oracle's fp32 operation sequence, every pixel
    // bit-identical to it at 4K.  SDF3D_PRECISION=fast opts into FMA
    // contraction and hardware sqrt/rcp: 1.47x faster on C4, but a few
    // grazing pixels end their march a step apart (C4: 48 pixels over 1e-4,
    // max 0.72; C5: 2,123, max 0.34; profiles/parity_fullsize.json)
    f.params.precision =
        env("SDF3D_PRECISION", "exact") == "fast" ? SDF_PRECISION_FAST : SDF_PRECISION_EXACT;
    if (std::getenv("WORLD_SIZE") || env("SDF3D_DRIVER", "0") == "1")
      return run_driver(f, frames, out);

    std::vector<sdf_material> materials;
    if (use_palette)
      materials = sdf::palette(f.scene.kind == SDF_SCENE_PRIMITIVES ? f.scene.count : 1);
    if ((use_palette || use_reflect || use_env || !projection.empty()) && lights.empty())
      lights.push_back(f.light);   // the reference's one light
    hipStream_t stream;
    sdf::check_hip(hipStreamCreate(&stream), "hipStreamCreate");
    hipEvent_t t0, t1;
    sdf::check_hip(hipEventCreate(&t0), "hipEventCreate");
    sdf::check_hip(hipEventCreate(&t1), "hipEventCreate");
    {
      sdf::Renderer r(W, H, stream);
      Navigator nav;
      // --projection: the frame's rays, n x 3 floats of origins and of directions
      const int64_t n = int64_t(W) * H;
      float *ray_o = nullptr, *ray_d = nullptr;
      if (!projection.empty()) {
        sdf::check_hip(hipMalloc(reinterpret_cast<void**>(&ray_o), size_t(n) * 12), "hipMalloc");
        sdf::check_hip(hipMalloc(reinterpret_cast<void**>(&ray_d), size_t(n) * 12), "hipMalloc");
      }
      if (projection == "equirect") {
        // pixel (x, y)'s centre: longitude -pi .. pi across (0 looks along -z),
        // latitude -pi/2 .. pi/2 up; any length will do, the kernel normalises
        const double pi = 3.14159265358979323846;
        std::vector<float> d(size_t(n) * 3);
        for (int y = 0; y < H; ++y)
          for (int x = 0; x < W; ++x) {
            const double lon = ((2.0 * x + 1.0) / W - 1.0) * pi;
            const double lat = ((2.0 * y + 1.0) / H - 1.0) * (pi / 2);
            float* q = &d[(size_t(y) * W + x) * 3];
            q[0] = float(std::cos(lat) * std::sin(lon));
            q[1] = float(std::sin(lat));
            q[2] = float(-std::cos(lat) * std::cos(lon));
          }
        sdf::check_hip(hipMemcpy(ray_d, d.data(), d.size() * 4, hipMemcpyHostToDevice),
                       "hipMemcpy");
      }
      for (int i = 0; i < frames; ++i) {
        nav.frame(f, i, frames);
        sdf::check_hip(hipEventRecord(t0, stream), "hipEventRecord");
        if (!projection.empty()) {
          // the camera's place per pixel, and for a pinhole the render's own rays
          const bool pinhole = projection == "pinhole";
          sdf::camera_rays(f, ray_o, pinhole ? ray_d : nullptr, stream);
          sdf::render_rays(f, lights, light_flags, materials, use_reflect ? &reflect : nullptr,
                           use_env ? &environment : nullptr, ray_o, ray_d, n, pinhole,
                           r.device_rgba(), nullptr, stream);
        } else if (use_env) r.render(f, lights, light_flags, materials, reflect, environment);
        else if (use_reflect) r.render(f, lights, light_flags, materials, reflect);
        else if (use_palette) r.render(f, lights, light_flags, materials);
        else if (lights.empty()) r.render(f);
        else r.render(f, lights, light_flags);
        sdf::check_hip(hipEventRecord(t1, stream), "hipEventRecord");
        sdf::check_hip(hipEventSynchronize(t1), "hipEventSynchronize");
        float ms = 0;
        sdf::check_hip(hipEventElapsedTime(&ms, t0, t1), "hipEventElapsedTime");
        std::printf("frame %d: %.3f ms (%.1f Mpixels/s)\n", i, ms, W * H / (ms * 1e3));
      }
      sdf::write_ppm(out, r.download(), W, H);
      (void)hipFree(ray_o);
      (void)hipFree(ray_d);
    }
    if (use_pick) {
      sdf::Frame q = f;          // the last frame's camera, one ray per pixel
      q.params.samples = 0;
      const sdf::Hit h = sdf::pick(q, pick_x, pick_y, stream);
      std::printf("pick %d,%d: %.9g %d %d %.9g %.9g %.9g\n", pick_x, pick_y, h.t, h.steps, h.prim,
                  h.normal[0], h.normal[1], h.normal[2]);
    }
    if (!mesh_path.empty()) {
      const double lo[3] = {box[0], box[1], box[2]}, hi[3] = {box[3], box[4], box[5]};
      const sdf_grid g = sdf::box_grid(lo, hi, mesh_n);
      const sdf::Mesh m =
          sdf::extract_mesh(f, g, true, false, stream, use_mesh_sharp ? &mesh_sharp : nullptr);
      std::vector<float> colors;
      if (mesh_colors) colors = sdf::bake(f, m, g, lights, light_flags, materials, nullptr, -1.0f, stream);
      const bool ply = mesh_path.size() > 4 && mesh_path.compare(mesh_path.size() - 4, 4, ".ply") == 0;
      if (ply) sdf::write_ply(mesh_path, m, colors);
      else sdf::write_obj(mesh_path, m, colors);
      std::printf("mesh: %lld vertices, %lld triangles, %lld of %lld bricks evaluated; wrote %s\n",
                  (long long)m.counts[0], (long long)m.counts[1], (long long)m.counts[2],
                  (long long)m.counts[3], mesh_path.c_str());
    }
    if (measure_n > 0) {
      // one JSON line: the solid inside the box on N cells per axis (sdf::measure);
      // with --density a density per primitive weighs mass, centroid and inertia
      const double lo[3] = {measure_box[0], measure_box[1], measure_box[2]},
                   hi[3] = {measure_box[3], measure_box[4], measure_box[5]};
      const sdf::Measure m = sdf::measure(f, sdf::box_grid(lo, hi, measure_n), !densities.empty(), stream);
      double c[3], I[3][3], blo[3], bhi[3];
      const double mass = densities.empty() ? m.volume() : m.mass(densities);
      std::printf("{\"measure\": {\"volume\": %.17g, \"mass\": %.17g, ", m.volume(), mass);
      // nothing weighs anything (an empty solid, densities of 0): no centroid and no
      // inertia, null as the bounds of an empty solid are (0 / 0 is no JSON number)
      if (m.moments(densities).m0 != 0.0) {
        m.centroid(c, densities);
        m.inertia(I, 1.0, densities);
        std::printf("\"centroid\": [%.17g, %.17g, %.17g], "
                    "\"inertia\": [[%.17g, %.17g, %.17g], [%.17g, %.17g, %.17g], [%.17g, %.17g, %.17g]], ",
                    c[0], c[1], c[2], I[0][0], I[0][1], I[0][2], I[1][0], I[1][1], I[1][2], I[2][0],
                    I[2][1], I[2][2]);
      } else {
        std::printf("\"centroid\": null, \"inertia\": null, ");
      }
      if (m.bounds(blo, bhi))
        std::printf("\"bounds\": [[%.17g, %.17g, %.17g], [%.17g, %.17g, %.17g]], ", blo[0], blo[1], blo[2],
                    bhi[0], bhi[1], bhi[2]);
      else
        std::printf("\"bounds\": null, ");
      std::printf("\"bricks\": {\"evaluated\": %lld, \"closed_form\": %lld, \"all\": %lld}}}\n",
                  (long long)m.counts[0], (long long)m.counts[1], (long long)m.counts[2]);
    }
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
    (void)hipStreamDestroy(stream);
    std::printf("wrote %s\n", out.c_str());
  } catch (const std::exception& e) {
    std::fprintf(stderr, "sdf_main: %s\n", e.what());
    return 1;
  }
  return 0;
}
