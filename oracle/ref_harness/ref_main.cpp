// ref_main.cpp -- drives the reference's own LBM_d3q19.H / LBM_binary.H, compiled against amrex_lite.H.
// TEST INFRASTRUCTURE ONLY.  Reads a request (text, one "key values..." per line; doubles in any form strtod
// reads, the Python side writes C99 hex floats), writes raw little-endian doubles in the project's [c][z][y][x] order.
//
//   mode run | unit | noise
//   n NX NY NZ
//   tau_f T   tau_g T   alpha0 A   alpha1 A   kappa K   kBT E      (the reference's mutable globals)
//   out PATH
//   normals PATH         table of doubles RandomNormal hands out in call order (absent: every normal is 0)
//   com X Y Z            what update_com returns; may repeat: call k gets line k, the last line serves all later calls
//   com_ref X Y Z        com_ref[0] of LBM_init / LBM_timestep
//   refstate PATH        rho_eq, phi_eq, rhot_eq, each [z][y][x] (read by the -DUSE_REF_STATE build only)
// mode run:
//   init stripe FRAC | droplet R | mixture | file      (file: LBM_init from `state`)
//   state PATH           f0 then g0, each [19][z][y][x]
//   steps N
//   dump S0 S1 ...       after these step counts (0 = after the init): f, g, hydrovsbar(15), hydrovs(22), fnoisevs, gnoisevs
//   It prints total mass, rho(0,0,4 % nz) and ufz(0,0,2 % nz) of the final state with 17 digits.
// mode noise:            thermal_noise alone
//   hbar PATH            rho then phi, each [z][y][x] -> hydrovsbar comps 0, 1
//   shift X Y Z          pos_com_relative
//   output: fnoisevs, gnoisevs
// mode unit:             the site functions on supplied inputs
//   count K
//   unit PATH            vec[K][19], fields[K][2], u[K][3], a[K][3], field[z][y][x]
//   output: moments[K][19], populations[K][19], equilibrium_moments index 0 [K][19] and index 1 [K][19],
//           phi_moments index 0 [K][19] and index 1 [K][19], gradient[3][z][y][x], grad_laplacian_2nd[3][z][y][x]
#include "amrex_lite.H"

#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

// The reference's update_com lives in LBM_hydrovs.H, which needs Eigen; its Debug.H and AMReX_FileIO.H need the full
// AMReX.  Their include guards are defined here so that LBM_binary.H's #include lines of them expand to nothing, and
// update_com returns what the request prescribes.
#define LBM_DEB_
#define LBM_IO_
#define LBM_HYDRO_
static std::vector<RealVect> g_com(1);
static std::size_t g_com_calls = 0;
inline void update_com(const Geometry&, RealVect& pos, MultiFab&) {
  pos = g_com[g_com_calls < g_com.size() ? g_com_calls : g_com.size() - 1];
  ++g_com_calls;
}

#include "LBM_binary.H"

namespace {

[[noreturn]] void die(const std::string& msg) {
  std::fprintf(stderr, "ref_main: %s\n", msg.c_str());
  std::exit(2);
}

std::vector<double> read_doubles(const std::string& path) {
  std::ifstream in(path, std::ios::binary | std::ios::ate);
  if (!in) die("cannot open " + path);
  const std::streamsize bytes = in.tellg();
  in.seekg(0);
  std::vector<double> v((std::size_t)bytes / sizeof(double));
  in.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(double)));
  return v;
}

double number(std::istringstream& s, const std::string& key) {
  std::string tok;
  if (!(s >> tok)) die("missing value for " + key);
  char* end = nullptr;
  const double v = std::strtod(tok.c_str(), &end);
  if (end == tok.c_str() || *end) die("bad number '" + tok + "' for " + key);
  return v;
}

RealVect vector3(std::istringstream& s, const std::string& key) {
  const double x = number(s, key), y = number(s, key), z = number(s, key);
  return RealVect(x, y, z);
}

struct Request {
  std::string mode = "run", init = "stripe", out, normals, state, refstate, hbar, unit;
  int n[3] = {0, 0, 0}, steps = 0, count = 0;
  double init_arg = 0.5;
  std::vector<int> dump;
  RealVect com_ref, shift;
};

struct Writer {
  std::FILE* fp;
  int nx, ny, nz;
  void field(MultiFab& m) {
    Array4<Real> a = m.view();
    for (int c = 0; c < m.nComp(); ++c)
      for (int z = 0; z < nz; ++z) for (int y = 0; y < ny; ++y) for (int x = 0; x < nx; ++x) {
        const double v = a(x, y, z, c);
        std::fwrite(&v, sizeof v, 1, fp);
      }
  }
  void values(const double* v, std::size_t n) { std::fwrite(v, sizeof(double), n, fp); }
};

// fills comps [c0, c0 + ncomp) of the valid cells from p[ncomp][z][y][x]
void fill(MultiFab& m, const double* p, int c0, int ncomp, int nx, int ny, int nz) {
  Array4<Real> a = m.view();
  for (int c = 0; c < ncomp; ++c)
    for (int z = 0; z < nz; ++z) for (int y = 0; y < ny; ++y) for (int x = 0; x < nx; ++x)
      a(x, y, z, c0 + c) = p[(((std::size_t)c * nz + z) * ny + y) * nx + x];
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) die("usage: ref_main REQUEST");
  std::ifstream rq(argv[1]);
  if (!rq) die(std::string("cannot open ") + argv[1]);
  Request r;
  bool have_com = false;
  for (std::string line; std::getline(rq, line);) {
    std::istringstream s(line);
    std::string key;
    if (!(s >> key) || key[0] == '#') continue;
    if (key == "mode") s >> r.mode;
    else if (key == "n") s >> r.n[0] >> r.n[1] >> r.n[2];
    else if (key == "tau_f") tau_f = number(s, key);
    else if (key == "tau_g") tau_g = number(s, key);
    else if (key == "alpha0") alpha0 = number(s, key);
    else if (key == "alpha1") alpha1 = number(s, key);
    else if (key == "kappa") kappa = number(s, key);
    else if (key == "kBT") kBT = number(s, key);
    else if (key == "out") s >> r.out;
    else if (key == "normals") s >> r.normals;
    else if (key == "state") s >> r.state;
    else if (key == "refstate") s >> r.refstate;
    else if (key == "hbar") s >> r.hbar;
    else if (key == "unit") s >> r.unit;
    else if (key == "count") s >> r.count;
    else if (key == "steps") s >> r.steps;
    else if (key == "dump") { for (int v; s >> v;) r.dump.push_back(v); }
    else if (key == "init") { s >> r.init; if (r.init == "stripe" || r.init == "droplet") r.init_arg = number(s, key); }
    else if (key == "com") { const RealVect v = vector3(s, key); if (have_com) g_com.push_back(v); else g_com[0] = v; have_com = true; }
    else if (key == "com_ref") r.com_ref = vector3(s, key);
    else if (key == "shift") r.shift = vector3(s, key);
    else die("unknown key " + key);
  }
  const int nx = r.n[0], ny = r.n[1], nz = r.n[2];
  if (nx < 1 || ny < 1 || nz < 1) die("n: three extents >= 1");
  if (r.out.empty()) die("no out");
  const std::size_t ns = (std::size_t)nx * ny * nz;

  std::vector<double> normals;
  if (!r.normals.empty()) {
    normals = read_doubles(r.normals);
    normal_table().v = normals.data();
    normal_table().n = normals.size();
  }

  Geometry geom;
  geom.dom = Box(IntVect(0, 0, 0), IntVect(nx - 1, ny - 1, nz - 1));
  MultiFab f(geom.dom, nvel), g(geom.dom, nvel), fnew(geom.dom, nvel), gnew(geom.dom, nvel);
  MultiFab h(geom.dom, 22), hb(geom.dom, 15), fn(geom.dom, nvel), gn(geom.dom, nvel);
  MultiFab rho_eq(geom.dom, 1), phi_eq(geom.dom, 1), rhot_eq(geom.dom, 1);
  amrex::Vector<RealVect> com_ref(1, r.com_ref);
  if (!r.refstate.empty()) {
    const std::vector<double> v = read_doubles(r.refstate);
    if (v.size() != 3 * ns) die("refstate: expected rho_eq, phi_eq, rhot_eq of the lattice");
    fill(rho_eq, v.data(), 0, 1, nx, ny, nz);
    fill(phi_eq, v.data() + ns, 0, 1, nx, ny, nz);
    fill(rhot_eq, v.data() + 2 * ns, 0, 1, nx, ny, nz);
  }

  std::FILE* fp = std::fopen(r.out.c_str(), "wb");
  if (!fp) die("cannot write " + r.out);
  Writer w{fp, nx, ny, nz};

  if (r.mode == "run") {
    if (r.init == "stripe") LBM_init_stripe(r.init_arg, geom, f, g, h, hb, fn, gn, rho_eq, phi_eq, rhot_eq);
    else if (r.init == "droplet") LBM_init_droplet(r.init_arg, geom, f, g, h, hb, fn, gn, rho_eq, phi_eq, rhot_eq);
    else if (r.init == "mixture") LBM_init_mixture(geom, f, g, h, hb, fn, gn, rho_eq, phi_eq, rhot_eq);
    else if (r.init == "file") {
      const std::vector<double> v = read_doubles(r.state);
      if (v.size() != 2 * nvel * ns) die("state: expected f0 and g0 of the lattice");
      MultiFab f0(geom.dom, nvel), g0(geom.dom, nvel);
      fill(f0, v.data(), 0, nvel, nx, ny, nz);
      fill(g0, v.data() + nvel * ns, 0, nvel, nx, ny, nz);
      LBM_init(geom, f, g, h, hb, fn, gn, f0, g0, rho_eq, phi_eq, rhot_eq, com_ref);
    } else die("unknown init " + r.init);
    for (int t = 0; t <= r.steps; ++t) {
      if (t) LBM_timestep(geom, f, g, fnew, gnew, h, hb, fn, gn, rho_eq, phi_eq, rhot_eq, com_ref);
      for (int d : r.dump)
        if (d == t) { w.field(f); w.field(g); w.field(hb); w.field(h); w.field(fn); w.field(gn); }
    }
    Array4<Real> a = hb.view(), hh = h.view();
    double mass = 0;
    for (int z = 0; z < nz; ++z) for (int y = 0; y < ny; ++y) for (int x = 0; x < nx; ++x) mass += a(x, y, z, 0) + a(x, y, z, 1);
    std::printf("mass %.17g rho(0,0,4) %.17g ufz(0,0,2) %.17g\n", mass, a(0, 0, 4 % nz, 0), hh(0, 0, 2 % nz, 4));
  } else if (r.mode == "noise") {
    const std::vector<double> v = read_doubles(r.hbar);
    if (v.size() != 2 * ns) die("hbar: expected rho and phi of the lattice");
    fill(hb, v.data(), 0, 2, nx, ny, nz);
    thermal_noise(geom, fn, gn, rho_eq, phi_eq, rhot_eq, hb, r.shift);
    w.field(fn); w.field(gn);
  } else if (r.mode == "unit") {
    const std::size_t K = (std::size_t)r.count;
    const std::vector<double> v = read_doubles(r.unit);
    if (v.size() != K * (19 + 2 + 3 + 3) + ns) die("unit: expected vec[K][19], fields[K][2], u[K][3], a[K][3], field[z][y][x]");
    const double *vec = v.data(), *fields = vec + 19 * K, *u = fields + 2 * K, *acc = u + 3 * K, *fld = acc + 3 * K;
    std::vector<double> o(K * 19);
    auto put = [&](std::size_t k, const Array1D<Real, 0, nvel>& m) { for (int i = 0; i < nvel; ++i) o[k * 19 + i] = m(i); };
    auto get = [&](std::size_t k) { Array1D<Real, 0, nvel> m; for (int i = 0; i < nvel; ++i) m(i) = vec[k * 19 + i]; return m; };
    for (std::size_t k = 0; k < K; ++k) put(k, moments(get(k)));
    w.values(o.data(), o.size());
    for (std::size_t k = 0; k < K; ++k) put(k, populations(get(k)));
    w.values(o.data(), o.size());
    for (int which = 0; which < 2; ++which)
      for (int idx = 0; idx < 2; ++idx) {
        for (std::size_t k = 0; k < K; ++k) {
          const Array1D<Real, 0, 2> fl = {fields[2 * k], fields[2 * k + 1]};
          const RealVect uu(u[3 * k], u[3 * k + 1], u[3 * k + 2]), aa(acc[3 * k], acc[3 * k + 1], acc[3 * k + 2]);
          put(k, which == 0 ? equilibrium_moments(fl, idx, uu) : phi_moments(fl, idx, uu, aa));
        }
        w.values(o.data(), o.size());
      }
    MultiFab s(geom.dom, 1), out3(geom.dom, 3);
    fill(s, fld, 0, 1, nx, ny, nz);
    s.FillBoundary(geom.periodicity());
    Array4<Real> sa = s.view(), oa = out3.view();
    for (int which = 0; which < 2; ++which) {
      for (int z = 0; z < nz; ++z) for (int y = 0; y < ny; ++y) for (int x = 0; x < nx; ++x) {
        const RealVect gv = which == 0 ? gradient(x, y, z, sa, 0) : grad_laplacian_2nd(x, y, z, sa, 0);
        for (int d = 0; d < 3; ++d) oa(x, y, z, d) = gv[d];
      }
      w.field(out3);
    }
  } else die("unknown mode " + r.mode);
  std::fclose(fp);
  return 0;
}
