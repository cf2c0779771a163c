// The lattice a uniform rectangle mesh's H1Space lives on, for the lattice sweeps of the whole-domain WaveHoltz solver
// (waveholtz.hpp, csrc/kernels/wave_lattice.hip).  Plain host code: nothing here touches the device.
//
// A mesh qualifies when its elements are axis-aligned rectangles, congruent to 1e-12 of their size, and element e sits at
// (e % nx, e / nx) of a grid (mesh.hpp's uniform_rect numbering), nx read off the first row.  The mesh is detected from its
// corners, not described by the caller.  The dofs then form a lattice of Lx x Ly Gauss-Lobatto nodes, L = n (n_basis - 1) + 1,
// and node (i, j) of element (ex, ey) is lattice node (ex (n_basis - 1) + i, ey (n_basis - 1) + j).
#ifndef CUDDH_AMD_WAVE_LATTICE_HPP
#define CUDDH_AMD_WAVE_LATTICE_HPP

#include <vector>

#include "spaces.hpp"

namespace cuddh
{
    struct WaveLatticeMap
    {
        int nx = 0, ny = 0, n_basis = 0;
        int Lx = 0, Ly = 0;
        int stride = 0;           // doubles per lattice row: Lx rounded up to even (rows start on 16-byte boundaries)
        double hx = 0.0, hy = 0.0;
        std::vector<int> node_of; // dof -> I + Lx J, a bijection onto [0, Lx Ly) (with missing cells: an injection)
        std::vector<unsigned char> cell; // empty: every cell exists; else nx ny flags, 1 where cell i + nx j exists

        int slots() const { return stride * Ly; }
        /// dof -> slot I + stride J of the padded vectors
        int slot_of(int dof) const { return node_of[dof] % Lx + stride * (node_of[dof] / Lx); }
    };

    /// From arrays alone: I (n_basis, n_basis, n_elem) element node -> dof; corners (2, 4, n_elem), the images of the reference
    /// corners (-1,-1), (1,-1), (1,1), (-1,1); xy (2, ndof) collocation points and x (n_basis) the reference nodes in [-1, 1],
    /// against which the local node order of the first and the last element is checked.  Verifies that the map is a bijection,
    /// that shared nodes agree and that ndof, Lx Ly and stride Ly fit in an int.  Anything else is refused through cuddh_error
    /// with a message that starts "WaveHoltz error: sweep:".
    WaveLatticeMap build_wave_lattice_map(int ndof, int n_elem, int n_basis, const int *I, const double *corners, const double *xy, const double *x);

    /// the same for a space (its coordinates are evaluated if they have not been)
    WaveLatticeMap build_wave_lattice_map(const H1Space &fem);

    /// A grid mesh with missing cells: the elements are a subset of the cells of a uniform nx x ny grid, listed in
    /// ascending cell index i + nx j with uniform_rect's corner order.  hx, hy come from element 0, the origin and nx, ny from the
    /// bounding box of all corners, an element's cell from its first corner.  Verified: every corner is where its cell has it (the
    /// tolerance of the full detection), cell indices strictly increase, shared nodes agree, node_of is injective, Lx Ly and
    /// stride Ly fit in an int.  `cell` is filled (all ones on a full grid); lattice nodes with no cell around them belong to no
    /// dof.  Anything else is refused through cuddh_error with a message that starts "WaveHoltz error: sweep:".
    WaveLatticeMap build_wave_cells_map(int ndof, int n_elem, int n_basis, const int *I, const double *corners, const double *xy, const double *x);
    WaveLatticeMap build_wave_cells_map(const H1Space &fem);

    /// What WaveHoltz's lattice form uses: the full detection, and only where that refuses the one with missing cells (whose
    /// refusal is then reported).  `cell` is empty exactly when the full detection accepted.
    WaveLatticeMap build_wave_lattice_or_cells_map(const H1Space &fem);

    /// A per-cell stiffness coefficient on the cell grid of `map`: h_beta holds n_elem values in element order, every
    /// one finite and positive.  On a full rectangle element e is cell e; on a grid with missing cells the present cells in
    /// ascending order take the values in element order and absent cells get 0.  Returns nx ny weights, cell (a, b) at a + nx b.
    /// A null h_beta, a value that is not finite and positive, or an n_elem that is not the map's number of cells is refused
    /// through cuddh_error with a message that starts "WaveHoltz error: cell_stiffness:".
    std::vector<double> wave_lattice_cell_weights(const WaveLatticeMap &map, int n_elem, const double *h_beta);

    /// the check of h_beta alone (what wave_lattice_cell_weights refuses about the values)
    void check_cell_stiffness(int n_elem, const double *h_beta);

    /// The time ratio a two-parameter medium asks for: the local wave speed is sqrt(beta) / a, and the ratio is
    /// max(1, ceil((1 - 1e-9) max_e (sqrt(beta_e) / min_{g in e} a_g))).  I (nodes_per_elem, n_elem): element node -> dof; h_a the
    /// nodal coefficient; h_beta n_elem values, or null for beta == 1, which is max(1, ceil((1 - 1e-9) / min a)) over the dofs of the
    /// elements.  A ratio above DDHTimeStep::max_ratio is refused through cuddh_error ("WaveHoltz error: time step: ...").
    int wave_coefficient_ratio(int n_elem, int nodes_per_elem, const int *I, const double *h_a, const double *h_beta);

    /// the 1-D tables of the Kronecker form on the reference element [-1, 1]: A = D^T diag(w) D (row-major, n_basis x n_basis), D the
    /// collocation derivative matrix, and the Gauss-Lobatto weights w
    void wave_lattice_tables(const Basis &basis, double *A, double *w);
} // namespace cuddh

#endif
