// bflbm_collide_body.inc -- the body of pass B of the two-pass schedule (pull, project, draw noise, collide, store),
// included verbatim by k_collide (bflbm_kernels.h) and by the replica-batch kernel (bflbm_batch.h), so that both
// compile the same source and the single-lattice kernel's instructions stay exactly what they were.
// In scope: NOISE, INJECT, UNIT (compile-time; UNIT: both relaxation rates are 1.0, see d_relax_with); S, D, rho, phi, injf,
// injg, G, P, p0, noise_index, Rf.
  __shared__ double ntab[(NOISE && !INJECT) ? BFLBM_NORMAL_TABLE_N : 4];
  if (NOISE && !INJECT) d_load_normal_table(ntab, true);
  BFLBM_SITE_FROM_BLOCK_XCD();
  SiteOff I; site_offsets(G, x, y, p, I);
  double fs[Q], gs[Q];
  pull_site(S, G, I, fs, gs);
  const double r = ld_sb(rho + I.pl[1], I.o[1][1]), ph = ld_sb(phi + I.pl[1], I.o[1][1]);
  double nb[Q], grad_rho[3], grad_phi[3];
  gather_field(rho, I, nb); d_gradient(P, nb, grad_rho);
  gather_field(phi, I, nb); d_gradient(P, nb, grad_phi);
  double* __restrict__ Dp = D + I.pl[1];
  unsigned o = I.o[1][1];
  // noise: the momentum modes first (the projection needs them), each fluid's other modes right before
  // its relaxation; every fluid is stored as soon as it is collided -- keeps the live set small
  const long long nvol = (long long)(G.nzs - 2*G.H)*G.dplane;         // injected arrays, dense: [a][p-H][y][x]
  const long long no = (long long)(p - G.H)*G.dplane + (long long)y*G.nx + x;
  double fn3[3] = {0., 0., 0.}, gn3[3] = {0., 0., 0.};
  NoiseAmp NA; bflbm_rng_state rst;
  if (INJECT) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { fn3[k] = injf[(1 + k)*nvol + no]; gn3[k] = injg[(1 + k)*nvol + no]; }
  } else if (NOISE) {
    double ar, ap, at;
    noise_state(Rf, G, x, y, p, r, ph, ar, ap, at);
    d_noise_amp(P, ar, ap, at, NA);
    d_noise_head(P, NA, global_site(G, x, y, p), noise_index, ntab, rst, fn3);
#pragma unroll
    for (int k = 0; k < 3; ++k) gn3[k] = -fn3[k];
  }
  SiteHydro Hy;
  SiteRecip R;
  d_site_recips(P, r, ph, R);
  {
    double jf[3], jg[3];
    d_momentum(fs, jf);
    d_momentum(gs, jg);
    d_hydrovars_j(P, jf, jg, r, ph, grad_rho, grad_phi, fn3, gn3, Hy, R);
  }
  double v_b[3];
  d_barycentric(r, ph, Hy, v_b, R);
  {
    double m[Q];
    d_moments(fs, m);
    if (INJECT) {
      double fn[Q];
#pragma unroll
      for (int a = 0; a < Q; ++a) fn[a] = injf[a*nvol + no];
      d_relax<true>(P, m, r, v_b, Hy.uf, Hy.af, P.inv_tau_f_bar, fn, R.cs4);
    } else if (NOISE) {
      d_relax_generated(P, m, r, v_b, Hy.uf, Hy.af, P.inv_tau_f_bar, fn3, NA.sr, ntab, rst, R.cs4);
    } else {
      const double zn[Q] = {0.};
      d_relax<false, UNIT>(P, m, r, v_b, Hy.uf, Hy.af, P.inv_tau_f_bar, zn, R.cs4);
    }
    d_populations(m, fs);
#pragma unroll
    for (int i = 0; i < Q; ++i) st_pop(Dp + (long long)i*G.vol, o, fs[i]);
  }
  {
    double m[Q];
    d_moments(gs, m);
    if (INJECT) {
      double gn[Q];
#pragma unroll
      for (int a = 0; a < Q; ++a) gn[a] = injg[a*nvol + no];
      d_relax<true>(P, m, ph, v_b, Hy.ug, Hy.ag, P.inv_tau_g_bar, gn, R.cs4);
    } else if (NOISE) {
      d_relax_generated(P, m, ph, v_b, Hy.ug, Hy.ag, P.inv_tau_g_bar, gn3, NA.sp, ntab, rst, R.cs4);
    } else {
      const double zn[Q] = {0.};
      d_relax<false, UNIT>(P, m, ph, v_b, Hy.ug, Hy.ag, P.inv_tau_g_bar, zn, R.cs4);
    }
    d_populations(m, gs);
#pragma unroll
    for (int i = 0; i < Q; ++i) st_pop(Dp + (long long)(i+Q)*G.vol, o, gs[i]);
  }
