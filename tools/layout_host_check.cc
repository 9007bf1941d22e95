// The host derivation of the device layout (csrc/layout_derive.cc) under the host sanitizers, no
// GPU: data/pore_pnp/pore.msh refined twice, the front half and every derived block for 1 and 3
// ranks at degrees 1 and 2, with the default knobs and with each one switched.  Exits 0; a
// sanitizer report aborts.  Built and run by `make -C dune-pnp_amd layout_host_check`.
#include <cstdio>
#include <string>

#include "layout_derive.h"

int main(int argc, char **argv) {
  const std::string path = argc > 1 ? argv[1] : "../data/pore_pnp/pore.msh";
  pnp::Mesh m0;
  std::string err;
  if (!pnp::read_gmsh(path, m0, err)) {
    std::fprintf(stderr, "%s: %s\n", path.c_str(), err.c_str());
    return 2;
  }
  m0 = pnp::refine(m0, 2);
  long long checked = 0;
  for (int degree = 1; degree <= 2; degree++)
    for (int nranks : {1, 3})
      for (int rank = 0; rank < nranks; rank++) {
        pnp::Mesh mesh = m0, tmesh;
        pnp::PkSpace pks;
        pnp::Fans fans;
        pnp::LocalLayout L;
        if (!pnp::validate(mesh, err) ||
            !pnp::build_host_layout(mesh, degree, rank, nranks, tmesh, pks, fans, L, err)) {
          std::fprintf(stderr, "P%d rank %d of %d: %s\n", degree, rank, nranks, err.c_str());
          return 1;
        }
        for (int k = -1; k < 6; k++) {
          pnp::LayoutKnobs K;
          if (k == 0) K.split_sort = false;
          if (k == 1) K.blkmap = false;
          if (k == 2) K.spmv_lds = false;
          if (k == 3) K.list_own_last = false;
          if (k == 4) K.halo_overlap = false;
          if (k == 5) K.xcd_remap = 1;
          pnp::DerivedLayout D;
          if (!pnp::derive_layout(mesh, L, K, D, err)) {
            std::fprintf(stderr, "P%d rank %d of %d: %s\n", degree, rank, nranks, err.c_str());
            return 1;
          }
          checked += (long long)D.spmv.ulist.size() + (long long)D.halo.boundary.size();
          const pnp::KeptLayout H = pnp::keep_layout(std::move(D));
          checked += (long long)H.blkmap.size() + H.lslots_live + H.uslots_live;
        }
      }
  std::printf("layout_host_check: ok (%lld)\n", checked);
  return 0;
}
