// bflbm_fused_body.inc -- the body of the fused plane-marching kernel (schedule 1), included verbatim by k_fused
// (bflbm_fused.h) and by the replica-batch kernel (bflbm_batch.h), so that both compile the same source and the
// single-lattice kernel's instructions stay exactly what they were.
// In scope: TX, TY, MODE, UNIT (compile-time; UNIT: both relaxation rates are 1.0, see d_relax_with); S, D, injf, injg, G, P,
// F, noise_index; the macro
// BFLBM_FUSED_MAP(col, chunk), which sets this workgroup's tile column and chunk and is false when it has none.
  static_assert((TX * TY) % 64 == 0, "whole waves");
  constexpr int LW = TX + 2;                     // LDS row length
  constexpr int LSZ = (TX + 2) * (TY + 2);
  constexpr int NW = TX * TY / 64;
  static_assert(NW % 2 == 0 && (2 * (TX + 2) + 2 * TY) <= 64 * (NW / 2), "ring tasks of one fluid must fit one per lane of half the waves");
  __shared__ double rp[4][2][LSZ];               // ring of 4 planes x {rho,phi} x (TY+2)x(TX+2)
  __shared__ double gl[Q][TX * TY];              // g populations of the previous plane
  __shared__ double ntab[MODE == 1 ? BFLBM_NORMAL_TABLE_N : 4];
  __shared__ double n3l[3][MODE == 1 ? TX * TY : 1];   // MODE 1: momentum-mode noise of the site being collided (thread-private column)
  if (MODE == 1) d_load_normal_table(ntab, true);

  int col, chunk;
  if (!BFLBM_FUSED_MAP(col, chunk)) return;   // whole workgroup leaves together
  const int tix = col % F.ntx, tiy = col / F.ntx;
  const int x0 = tix * TX, y0 = tiy * TY;
  const int aw = min(TX, G.nx - x0), ah = min(TY, G.ny - y0);   // active extent of this tile
  const int tid = threadIdx.x;
  const int tx = tid % TX, ty = tid / TX;
  auto wrapx = [&](int v) { return v < 0 ? v + G.nx : (v >= G.nx ? v - G.nx : v); };
  auto wrapy = [&](int v) { return v < 0 ? v + G.ny : (v >= G.ny ? v - G.ny : v); };

  // ---- own site: per-thread 32-bit element offsets inside a plane, fixed for the whole march
  const bool loader = (tx < aw) && (ty < ah);
  const bool interior = loader;
  const int x = loader ? x0 + tx : x0, y = loader ? y0 + ty : y0;
  // byte offsets: a plane is < 4 GB (checked at creation), so  address = wave-uniform base + 32-bit lane
  // offset  and the loads/stores use the scalar-base addressing form (no 64-bit per-lane address math)
  const unsigned xo[3] = { (unsigned)wrapx(x - 1) * 8u, (unsigned)x * 8u, (unsigned)wrapx(x + 1) * 8u };
  const unsigned yo[3] = { (unsigned)(wrapy(y - 1) * G.pitch) * 8u, (unsigned)(y * G.pitch) * 8u, (unsigned)(wrapy(y + 1) * G.pitch) * 8u };
  auto ld = [](const double* __restrict__ base, unsigned boff) { return *reinterpret_cast<const double*>(reinterpret_cast<const char*>(base) + boff); };
  // plain population stores (the non-temporal hint was +0.8 % at 256^3, -2.0 % at 512^3 in this kernel, profiles/r04_nt_hints.txt)
  auto st = [](double* __restrict__ base, unsigned boff, double v) { *reinterpret_cast<double*>(reinterpret_cast<char*>(base) + boff) = v; };
  // ---- ring half-task of this thread: lanes 0..nper-1 of every wave; the lower half of the waves sums
  // fluid f, the upper half fluid g, so the fluid (and with it the load base) is wave-uniform
  const int nring = 2 * (aw + 2) + 2 * ah;
  const int nper = (nring + NW / 2 - 1) / (NW / 2);
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hfl = wv / (NW / 2);
  const int task = (wv % (NW / 2)) * nper + lane;
  const bool has_task = lane < nper && task < nring;
  int hlx = 0, hly = 0;                          // LDS coordinates of the ring site
  if (has_task) {
    const int r = task;
    if (r < aw + 2) { hlx = r; hly = 0; }
    else if (r < 2 * (aw + 2)) { hlx = r - (aw + 2); hly = ah + 1; }
    else if (r < 2 * (aw + 2) + ah) { hlx = 0; hly = r - 2 * (aw + 2) + 1; }
    else { hlx = aw + 1; hly = r - 2 * (aw + 2) - ah + 1; }
  }
  const int hx = wrapx(x0 + hlx - 1);            // in [-1, nx]: one wrap suffices
  const int hy = wrapy(y0 + hly - 1);
  const unsigned hxo[3] = { (unsigned)wrapx(hx - 1) * 8u, (unsigned)hx * 8u, (unsigned)wrapx(hx + 1) * 8u };
  const unsigned hyo[3] = { (unsigned)(wrapy(hy - 1) * G.pitch) * 8u, (unsigned)(hy * G.pitch) * 8u, (unsigned)(wrapy(hy + 1) * G.pitch) * 8u };

  const int lown = (ty + 1) * LW + (tx + 1);
  const int lhalo = hly * LW + hlx;

  // ---- chunk of planes
  const int qa = F.pa + chunk * F.cstride;
  const int qb = min(F.pb, qa + F.lz);
  auto wrapp = [&](int q) {                      // q in [-2, nzs+1]; nzs may be 1, so use a true modulo
    if (!G.zwrap) return q;
    const int m = q % G.nzs;
    return m < 0 ? m + G.nzs : m;
  };

  // Held across one march position: f of the previous plane in registers, g of the previous
  // plane in LDS (each thread only touches its own column gl[.][tid], so no barrier is needed).
  double pf[Q];
#pragma unroll
  for (int i = 0; i < Q; ++i) pf[i] = 0.;

  int it = 0;
  for (int q = qa - 1; q <= qb; ++q, ++it) {
    const int slot = it & 3;
    // wave-uniform plane bases: every load below is  (SGPR base) + (32-bit lane offset)
    const double* __restrict__ pl[3] = { S + (long long)wrapp(q - 1) * G.plane, S + (long long)wrapp(q) * G.plane,
                                         S + (long long)wrapp(q + 1) * G.plane };
    // 1. pull plane q: the own site first, then the ring half-task (measured: +2.3 % over ring first);
    //    everything is in flight together
    double cf[Q], cg[Q];
    if (loader) {
      unsigned oo[3][3];
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b2 = 0; b2 < 3; ++b2) { oo[a][b2] = yo[a] + xo[b2]; asm volatile("" : "+v"(oo[a][b2])); }
#pragma unroll
      for (int i = 0; i < Q; ++i) {
        const double* __restrict__ b = pl[1 - Vel::cz[i]] + (long long)i * G.vol;
        const unsigned o = oo[1 - Vel::cy[i]][1 - Vel::cx[i]];
        cf[i] = ld(b, o);
        cg[i] = ld(b + (long long)Q * G.vol, o);
      }
    } else {
#pragma unroll
      for (int i = 0; i < Q; ++i) { cf[i] = 0.; cg[i] = 0.; }
    }
    double hv[Q];
    if (has_task) {
      // the nine (dy,dx) offsets as opaque 32-bit values INSIDE this block: instruction selection then sees
      // base + zext(offset) and uses the scalar-base addressing form instead of 64-bit per-lane adds
      unsigned ho[3][3];
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b2 = 0; b2 < 3; ++b2) { ho[a][b2] = hyo[a] + hxo[b2]; asm volatile("" : "+v"(ho[a][b2])); }
#pragma unroll
      for (int i = 0; i < Q; ++i) {
        const double* __restrict__ b = pl[1 - Vel::cz[i]] + (long long)hfl * Q * G.vol + (long long)i * G.vol;
        hv[i] = ld(b, ho[1 - Vel::cy[i]][1 - Vel::cx[i]]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < Q; ++i) hv[i] = 0.;
    }
    // 2. densities of plane q into the ring slot.  The sums start from an opaque zero defined HERE: with a
    // literal 0.0 the compiler sinks the first addition (0.0 + f_0) into the load blocks above and waits
    // for the first load before it issues the rest.
    double zero = 0.0;
    asm volatile("" : "+v"(zero));
    auto density = [&](const double (&fs)[Q]) { double r = zero;
#pragma unroll
      for (int i = 0; i < Q; ++i) r += fs[i];
      return r; };
    // own sums first: their loads were issued first, the ring loads are still landing meanwhile
    if (loader) { rp[slot][0][lown] = density(cf); rp[slot][1][lown] = density(cg); }
    if (has_task) rp[slot][hfl][lhalo] = density(hv);
    __syncthreads();
    // 3. collide plane q-1: f from registers, g streamed out of LDS while plane q's g takes its place
    const bool do_collide = (q - 1 >= qa) && (q - 1 < qb) && interior;
    double mg[Q], jg[3];
    if (do_collide) {
      double pg[Q];
#pragma unroll
      for (int i = 0; i < Q; ++i) pg[i] = gl[i][tid];
      d_moments(pg, mg);
      d_momentum(pg, jg);
    }
#pragma unroll
    for (int i = 0; i < Q; ++i) gl[i][tid] = cg[i];
    if (do_collide) {
      double mf[Q], jf[3];
      d_moments(pf, mf);
      d_momentum(pf, jf);
      const int sl[3] = { (it - 2) & 3, (it - 1) & 3, it & 3 };
      const double r = rp[sl[1]][0][lown], ph = rp[sl[1]][1][lown];
      double nb[Q], grad_rho[3], grad_phi[3];
#pragma unroll
      for (int i = 0; i < Q; ++i) nb[i] = rp[sl[1 + Vel::cz[i]]][0][lown + Vel::cy[i] * LW + Vel::cx[i]];
      d_gradient(P, nb, grad_rho);
#pragma unroll
      for (int i = 0; i < Q; ++i) nb[i] = rp[sl[1 + Vel::cz[i]]][1][lown + Vel::cy[i] * LW + Vel::cx[i]];
      d_gradient(P, nb, grad_phi);
      const int pc = wrapp(q - 1);
      // noise: momentum modes now (hydrovars needs them), the rest right before each relaxation
      double fn3[3] = {0., 0., 0.}, gn3[3] = {0., 0., 0.};
      NoiseAmp NA; bflbm_rng_state rst;
      const double* __restrict__ nb_f = nullptr; const double* __restrict__ nb_g = nullptr;
      long long nvol = 0; unsigned no = 0;
      if (MODE == 2) {
        nvol = (long long)(G.nzs - 2 * G.H) * G.dplane;          // injected arrays are dense
        nb_f = injf + (long long)(pc - G.H) * G.dplane;
        nb_g = injg + (long long)(pc - G.H) * G.dplane;
        no = (unsigned)(y * G.nx + x) * 8u;
#pragma unroll
        for (int k = 0; k < 3; ++k) { fn3[k] = ld(nb_f + (1 + k) * nvol, no); gn3[k] = ld(nb_g + (1 + k) * nvol, no); }
      } else if (MODE == 1) {
        d_noise_amp(P, r, ph, r + ph, NA);
        d_noise_head(P, NA, global_site(G, x, y, pc), noise_index, ntab, rst, fn3);
#pragma unroll
        for (int k = 0; k < 3; ++k) { gn3[k] = -fn3[k]; n3l[k][tid] = fn3[k]; }
      }
      double* __restrict__ Dp = D + (long long)pc * G.plane;
      unsigned o = yo[1] + xo[1];
      asm volatile("" : "+v"(o));
      {
        SiteHydro Hy;
        SiteRecip R;
        d_site_recips(P, r, ph, R);
        d_hydrovars_j(P, jf, jg, r, ph, grad_rho, grad_phi, fn3, gn3, Hy, R);
        double v_b[3];
        d_barycentric(r, ph, Hy, v_b, R);
        {
          if (MODE == 2) {
            double fn[Q];
#pragma unroll
            for (int a = 0; a < Q; ++a) fn[a] = ld(nb_f + a * nvol, no);
            d_relax<true>(P, mf, r, v_b, Hy.uf, Hy.af, P.inv_tau_f_bar, fn, R.cs4);
          } else if (MODE == 1) {
            const double n3[3] = { n3l[0][tid], n3l[1][tid], n3l[2][tid] };     // reloaded: keeps the register budget
            d_relax_generated(P, mf, r, v_b, Hy.uf, Hy.af, P.inv_tau_f_bar, n3, sqrt(fabs(r)), ntab, rst, R.cs4);
          } else {
            const double zn[Q] = {0.};
            d_relax<false, UNIT>(P, mf, r, v_b, Hy.uf, Hy.af, P.inv_tau_f_bar, zn, R.cs4);
          }
          double out[Q];
          d_populations(mf, out);
#pragma unroll
          for (int i = 0; i < Q; ++i) st(Dp + (long long)i * G.vol, o, out[i]);
        }
        {
          if (MODE == 2) {
            double gn[Q];
#pragma unroll
            for (int a = 0; a < Q; ++a) gn[a] = ld(nb_g + a * nvol, no);
            d_relax<true>(P, mg, ph, v_b, Hy.ug, Hy.ag, P.inv_tau_g_bar, gn, R.cs4);
          } else if (MODE == 1) {
            const double n3[3] = { -n3l[0][tid], -n3l[1][tid], -n3l[2][tid] };
            d_relax_generated(P, mg, ph, v_b, Hy.ug, Hy.ag, P.inv_tau_g_bar, n3, sqrt(fabs(ph)), ntab, rst, R.cs4);
          } else {
            const double zn[Q] = {0.};
            d_relax<false, UNIT>(P, mg, ph, v_b, Hy.ug, Hy.ag, P.inv_tau_g_bar, zn, R.cs4);
          }
          double out[Q];
          d_populations(mg, out);
#pragma unroll
          for (int i = 0; i < Q; ++i) st(Dp + (long long)(i + Q) * G.vol, o, out[i]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < Q; ++i) pf[i] = cf[i];
  }
