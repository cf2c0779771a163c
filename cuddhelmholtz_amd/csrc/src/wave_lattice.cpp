// Detection of the lattice behind a uniform rectangle mesh, or behind a grid mesh with missing cells: see cuddh/wave_lattice.hpp.  Plain C++: nothing here touches the device.
#include "cuddh/wave_lattice.hpp"

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <string>

#include "cuddh/ddh.hpp"

namespace cuddh
{
    namespace
    {
        // a refusal on its way to cuddh_error: build_wave_lattice_or_cells_map tries the second detection before anything is reported
        struct Refusal
        {
            std::string message;
        };
        [[noreturn]] void refuse(const std::string &why)
        {
            throw Refusal{"WaveHoltz error: sweep: the lattice form needs a uniform rectangle mesh (Mesh2D::uniform_rect's numbering); " + why};
        }
        [[noreturn]] void refuse_cells(const std::string &why)
        {
            throw Refusal{"WaveHoltz error: sweep: the lattice form needs a uniform rectangle mesh or a grid mesh with missing cells "
                          "(Mesh2D::grid_cells' numbering); " + why};
        }
        template <typename F>
        WaveLatticeMap reported(F &&detect)
        {
            try
            {
                return detect();
            }
            catch (const Refusal &r)
            {
                cuddh_error(r.message.c_str());
                throw std::logic_error("unreachable");
            }
        }

        struct SpaceArrays
        {
            int n_elem, nb;
            std::vector<double> corners, x;
            const int *I;
            const double *xy;
        };
        SpaceArrays arrays_of(const H1Space &fem)
        {
            const Mesh2D &mesh = fem.mesh();
            SpaceArrays a;
            a.n_elem = mesh.n_elem();
            a.nb = fem.basis().size();
            a.corners.resize(8 * static_cast<std::size_t>(a.n_elem));
            a.x.resize(a.nb);
            static const double ref[4][2] = {{-1.0, -1.0}, {1.0, -1.0}, {1.0, 1.0}, {-1.0, 1.0}};
            for (int e = 0; e < a.n_elem; ++e)
                for (int c = 0; c < 4; ++c)
                    mesh.element(e)->physical_coordinates(ref[c], a.corners.data() + 2 * (c + 4 * static_cast<std::size_t>(e)));
            for (int i = 0; i < a.nb; ++i)
                a.x[i] = fem.basis().quadrature().x(i);
            a.I = fem.global_indices(MemorySpace::HOST);
            a.xy = fem.physical_coordinates(MemorySpace::HOST);
            return a;
        }

        WaveLatticeMap full_map(int ndof, int n_elem, int nb, const int *I, const double *corners, const double *xy, const double *x);
        WaveLatticeMap cells_map(int ndof, int n_elem, int nb, const int *I, const double *corners, const double *xy, const double *x);
    } // namespace

    WaveLatticeMap build_wave_lattice_map(int ndof, int n_elem, int nb, const int *I, const double *corners, const double *xy, const double *x)
    {
        return reported([&] { return full_map(ndof, n_elem, nb, I, corners, xy, x); });
    }

    WaveLatticeMap build_wave_lattice_map(const H1Space &fem)
    {
        const SpaceArrays a = arrays_of(fem);
        return build_wave_lattice_map(fem.size(), a.n_elem, a.nb, a.I, a.corners.data(), a.xy, a.x.data());
    }

    WaveLatticeMap build_wave_cells_map(int ndof, int n_elem, int nb, const int *I, const double *corners, const double *xy, const double *x)
    {
        return reported([&] { return cells_map(ndof, n_elem, nb, I, corners, xy, x); });
    }

    WaveLatticeMap build_wave_cells_map(const H1Space &fem)
    {
        const SpaceArrays a = arrays_of(fem);
        return build_wave_cells_map(fem.size(), a.n_elem, a.nb, a.I, a.corners.data(), a.xy, a.x.data());
    }

    WaveLatticeMap build_wave_lattice_or_cells_map(const H1Space &fem)
    {
        const SpaceArrays a = arrays_of(fem);
        try
        {
            return full_map(fem.size(), a.n_elem, a.nb, a.I, a.corners.data(), a.xy, a.x.data());
        }
        catch (const Refusal &)
        {
        }
        return build_wave_cells_map(fem.size(), a.n_elem, a.nb, a.I, a.corners.data(), a.xy, a.x.data());
    }

    namespace
    {
    // (the two detections, at the indentation the first one had as build_wave_lattice_map: its text is unchanged)
    WaveLatticeMap full_map(int ndof, int n_elem, int nb, const int *I, const double *corners, const double *xy, const double *x)
    {
        if (ndof < 1 || n_elem < 1 || nb < 2 || !I || !corners || !xy || !x)
            refuse("the space is empty or an array is missing.");
        auto cx = [&](int e, int c) { return corners[2 * (c + 4 * e)]; };
        auto cy = [&](int e, int c) { return corners[2 * (c + 4 * e) + 1]; };

        WaveLatticeMap L;
        L.n_basis = nb;
        const double x0 = cx(0, 0), y0 = cy(0, 0);
        L.hx = cx(0, 1) - x0;
        L.hy = cy(0, 3) - y0;
        if (!(L.hx > 0.0) || !(L.hy > 0.0) || !std::isfinite(L.hx) || !std::isfinite(L.hy))
            refuse("element 0 does not run from its first corner to the right and upwards.");
        double big = 0.0; // the largest coordinate, for the rounding of the corners themselves
        for (int i = 0; i < 8 * n_elem; ++i)
            big = std::max(big, std::fabs(corners[i]));
        const double tol = 1e-12 * std::min(L.hx, L.hy) + 8.0 * DBL_EPSILON * big;
        auto near = [&](double a, double b) { return std::fabs(a - b) <= tol; }; // (false for a NaN)

        // nx: the elements of the first row
        int nx = 1;
        while (nx < n_elem && near(cy(nx, 0), y0) && near(cx(nx, 0), x0 + nx * L.hx))
            ++nx;
        if (n_elem % nx != 0)
            refuse(std::to_string(n_elem) + " elements do not fill rows of " + std::to_string(nx) + ".");
        const int ny = n_elem / nx;
        L.nx = nx;
        L.ny = ny;
        for (int e = 0; e < n_elem; ++e)
        {
            const double ax = x0 + (e % nx) * L.hx, ay = y0 + (e / nx) * L.hy;
            const double want[4][2] = {{ax, ay}, {ax + L.hx, ay}, {ax + L.hx, ay + L.hy}, {ax, ay + L.hy}};
            for (int c = 0; c < 4; ++c)
                if (!near(cx(e, c), want[c][0]) || !near(cy(e, c), want[c][1]))
                    refuse("corner " + std::to_string(c) + " of element " + std::to_string(e) + " is not where cell (" + std::to_string(e % nx) + ", " +
                           std::to_string(e / nx) + ") of a " + std::to_string(nx) + " x " + std::to_string(ny) + " grid has it.");
        }

        const int H = nb - 1;
        const long long Lx = static_cast<long long>(nx) * H + 1, Ly = static_cast<long long>(ny) * H + 1, stride = Lx + (Lx & 1);
        if (Lx * Ly > INT_MAX || stride * Ly > INT_MAX)
            refuse("its " + std::to_string(Lx) + " x " + std::to_string(Ly) + " nodes do not fit a 32-bit index.");
        if (Lx * Ly != ndof)
            refuse("the space has " + std::to_string(ndof) + " dofs, the lattice " + std::to_string(Lx * Ly) + " nodes.");
        L.Lx = static_cast<int>(Lx);
        L.Ly = static_cast<int>(Ly);
        L.stride = static_cast<int>(stride);

        // dof -> node, from the element positions; the nodes neighbouring elements share must agree
        L.node_of.assign(ndof, -1);
        for (int e = 0; e < n_elem; ++e)
            for (int j = 0; j < nb; ++j)
                for (int i = 0; i < nb; ++i)
                {
                    const int g = I[i + nb * (j + nb * e)];
                    if (g < 0 || g >= ndof)
                        refuse("a global index lies outside the space.");
                    const int node = (e % nx) * H + i + L.Lx * ((e / nx) * H + j);
                    if (L.node_of[g] >= 0 && L.node_of[g] != node)
                        refuse("dof " + std::to_string(g) + " is shared by element nodes that are not the same lattice node.");
                    L.node_of[g] = node;
                }
        std::vector<char> taken(ndof, 0);
        for (int g = 0; g < ndof; ++g)
        {
            if (L.node_of[g] < 0)
                refuse("dof " + std::to_string(g) + " belongs to no element.");
            if (taken[L.node_of[g]])
                refuse("two dofs are the same lattice node.");
            taken[L.node_of[g]] = 1;
        }

        // the local node order: node (i, j) of an element is its point (x[i], x[j]), i along x
        for (const int e : {0, n_elem - 1})
            for (int j = 0; j < nb; ++j)
                for (int i = 0; i < nb; ++i)
                {
                    const int g = I[i + nb * (j + nb * e)];
                    const double px = x0 + (e % nx) * L.hx + 0.5 * (x[i] + 1.0) * L.hx, py = y0 + (e / nx) * L.hy + 0.5 * (x[j] + 1.0) * L.hy;
                    if (!near(xy[2 * g], px) || !near(xy[2 * g + 1], py))
                        refuse("node (" + std::to_string(i) + ", " + std::to_string(j) + ") of element " + std::to_string(e) +
                               " is not at the collocation point the lattice gives it.");
                }
        return L;
    }

    WaveLatticeMap cells_map(int ndof, int n_elem, int nb, const int *I, const double *corners, const double *xy, const double *x)
    {
        if (ndof < 1 || n_elem < 1 || nb < 2 || !I || !corners || !xy || !x)
            refuse_cells("the space is empty or an array is missing.");
        auto cx = [&](int e, int c) { return corners[2 * (c + 4 * static_cast<std::size_t>(e))]; };
        auto cy = [&](int e, int c) { return corners[2 * (c + 4 * static_cast<std::size_t>(e)) + 1]; };

        WaveLatticeMap L;
        L.n_basis = nb;
        L.hx = cx(0, 1) - cx(0, 0);
        L.hy = cy(0, 3) - cy(0, 0);
        if (!(L.hx > 0.0) || !(L.hy > 0.0) || !std::isfinite(L.hx) || !std::isfinite(L.hy))
            refuse_cells("element 0 does not run from its first corner to the right and upwards.");
        double big = 0.0, x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
        for (int e = 0; e < n_elem; ++e)
            for (int c = 0; c < 4; ++c)
            {
                const double px = cx(e, c), py = cy(e, c);
                if (!std::isfinite(px) || !std::isfinite(py))
                    refuse_cells("a corner of element " + std::to_string(e) + " is not finite.");
                big = std::max(big, std::max(std::fabs(px), std::fabs(py)));
                x0 = std::min(x0, px);
                x1 = std::max(x1, px);
                y0 = std::min(y0, py);
                y1 = std::max(y1, py);
            }
        const double tol = 1e-12 * std::min(L.hx, L.hy) + 8.0 * DBL_EPSILON * big;
        auto near = [&](double a, double b) { return std::fabs(a - b) <= tol; };

        // nx, ny: the bounding box in cells
        const double fx = std::round((x1 - x0) / L.hx), fy = std::round((y1 - y0) / L.hy);
        const int H = nb - 1;
        if (!(fx >= 1.0) || !(fy >= 1.0) || fx * H + 2.0 > INT_MAX || fy * H + 2.0 > INT_MAX)
            refuse_cells("the bounding box is not a grid of cells of element 0's size that fits a 32-bit index.");
        const long long nx = static_cast<long long>(fx), ny = static_cast<long long>(fy);
        if (!near(x0 + nx * L.hx, x1) || !near(y0 + ny * L.hy, y1))
            refuse_cells("the bounding box is not a whole number of cells of element 0's size.");
        const long long Lx = nx * H + 1, Ly = ny * H + 1, stride = Lx + (Lx & 1);
        if (Lx * Ly > INT_MAX || stride * Ly > INT_MAX)
            refuse_cells("its " + std::to_string(Lx) + " x " + std::to_string(Ly) + " nodes do not fit a 32-bit index.");
        L.nx = static_cast<int>(nx);
        L.ny = static_cast<int>(ny);
        L.Lx = static_cast<int>(Lx);
        L.Ly = static_cast<int>(Ly);
        L.stride = static_cast<int>(stride);

        // every element is a cell, in ascending cell index
        std::vector<int> cell_of(n_elem);
        long long last = -1;
        for (int e = 0; e < n_elem; ++e)
        {
            const double gi = std::round((cx(e, 0) - x0) / L.hx), gj = std::round((cy(e, 0) - y0) / L.hy);
            if (!(gi >= 0.0 && gi < fx && gj >= 0.0 && gj < fy))
                refuse_cells("the first corner of element " + std::to_string(e) + " is not the first corner of a cell.");
            const int i = static_cast<int>(gi), j = static_cast<int>(gj);
            const double ax = x0 + i * L.hx, ay = y0 + j * L.hy;
            const double want[4][2] = {{ax, ay}, {ax + L.hx, ay}, {ax + L.hx, ay + L.hy}, {ax, ay + L.hy}};
            for (int c = 0; c < 4; ++c)
                if (!near(cx(e, c), want[c][0]) || !near(cy(e, c), want[c][1]))
                    refuse_cells("corner " + std::to_string(c) + " of element " + std::to_string(e) + " is not where cell (" + std::to_string(i) + ", " +
                                 std::to_string(j) + ") of a " + std::to_string(nx) + " x " + std::to_string(ny) + " grid has it.");
            const long long id = i + nx * j;
            if (id <= last)
                refuse_cells("element " + std::to_string(e) + " is cell " + std::to_string(id) + ", not beyond cell " + std::to_string(last) +
                             " of the element before it: the cells must come in ascending order, each once.");
            last = id;
            cell_of[e] = static_cast<int>(id);
        }

        // dof -> node, from the cells; the nodes neighbouring elements share must agree
        std::vector<int> node_of(ndof, -1);
        for (int e = 0; e < n_elem; ++e)
            for (int j = 0; j < nb; ++j)
                for (int i = 0; i < nb; ++i)
                {
                    const int g = I[i + nb * (j + nb * static_cast<std::size_t>(e))];
                    if (g < 0 || g >= ndof)
                        refuse_cells("a global index lies outside the space.");
                    const int node = (cell_of[e] % L.nx) * H + i + L.Lx * ((cell_of[e] / L.nx) * H + j);
                    if (node_of[g] >= 0 && node_of[g] != node)
                        refuse_cells("dof " + std::to_string(g) + " is shared by element nodes that are not the same lattice node.");
                    node_of[g] = node;
                }
        {
            std::vector<int> sorted(node_of);
            std::sort(sorted.begin(), sorted.end());
            if (sorted.front() < 0)
                refuse_cells("a dof belongs to no element.");
            if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
                refuse_cells("two dofs are the same lattice node.");
        }

        // the local node order: node (i, j) of an element is its point (x[i], x[j]), i along x
        for (const int e : {0, n_elem - 1})
            for (int j = 0; j < nb; ++j)
                for (int i = 0; i < nb; ++i)
                {
                    const int g = I[i + nb * (j + nb * static_cast<std::size_t>(e))];
                    const double px = x0 + (cell_of[e] % L.nx) * L.hx + 0.5 * (x[i] + 1.0) * L.hx;
                    const double py = y0 + (cell_of[e] / L.nx) * L.hy + 0.5 * (x[j] + 1.0) * L.hy;
                    if (!near(xy[2 * g], px) || !near(xy[2 * g + 1], py))
                        refuse_cells("node (" + std::to_string(i) + ", " + std::to_string(j) + ") of element " + std::to_string(e) +
                                     " is not at the collocation point the lattice gives it.");
                }
        L.cell.assign(static_cast<std::size_t>(L.nx) * L.ny, 0);
        for (int e = 0; e < n_elem; ++e)
            L.cell[cell_of[e]] = 1;
        L.node_of = std::move(node_of);
        return L;
    }
    } // namespace

    void check_cell_stiffness(int n_elem, const double *h_beta)
    {
        if (!h_beta || n_elem < 1)
            cuddh_error("WaveHoltz error: cell_stiffness: no values were given.");
        for (int e = 0; e < n_elem; ++e)
            if (!std::isfinite(h_beta[e]) || !(h_beta[e] > 0.0))
                cuddh_error(("WaveHoltz error: cell_stiffness: beta = " + std::to_string(h_beta[e]) + " at element " + std::to_string(e) +
                             "; beta must be finite and positive.").c_str());
    }

    std::vector<double> wave_lattice_cell_weights(const WaveLatticeMap &map, int n_elem, const double *h_beta)
    {
        check_cell_stiffness(n_elem, h_beta);
        const std::size_t n_cells = static_cast<std::size_t>(map.nx) * map.ny;
        const std::size_t present = map.cell.empty() ? n_cells : static_cast<std::size_t>(std::count(map.cell.begin(), map.cell.end(), 1));
        if (present != static_cast<std::size_t>(n_elem))
            cuddh_error(("WaveHoltz error: cell_stiffness: " + std::to_string(n_elem) + " values for the " + std::to_string(present) +
                         " cells of the grid.").c_str());
        std::vector<double> weights(n_cells, 0.0);
        if (map.cell.empty())
            std::copy(h_beta, h_beta + n_elem, weights.begin());
        else
        {
            // the elements are the present cells in ascending order (cells_map verifies it)
            int e = 0;
            for (std::size_t c = 0; c < n_cells; ++c)
                if (map.cell[c])
                    weights[c] = h_beta[e++];
        }
        return weights;
    }

    int wave_coefficient_ratio(int n_elem, int nodes_per_elem, const int *I, const double *h_a, const double *h_beta)
    {
        if (n_elem < 1 || nodes_per_elem < 1 || !I || !h_a)
            cuddh_error("WaveHoltz error: time step: the ratio needs the elements' nodes and the coefficient.");
        double speed = 0.0; // max over the elements of sqrt(beta) / min a
        for (int e = 0; e < n_elem; ++e)
        {
            double a_min = INFINITY;
            for (int k = 0; k < nodes_per_elem; ++k)
                a_min = std::min(a_min, h_a[I[k + static_cast<std::size_t>(nodes_per_elem) * e]]);
            speed = std::max(speed, (h_beta ? std::sqrt(h_beta[e]) : 1.0) / a_min);
        }
        const double steps = std::ceil(speed * (1.0 - 1e-9));
        if (!(steps <= DDHTimeStep::max_ratio))
            cuddh_error(("WaveHoltz error: time step: max sqrt(beta) / a = " + std::to_string(speed) + " asks for more than " +
                         std::to_string(DDHTimeStep::max_ratio) + " times the mesh grid's steps.").c_str());
        return std::max(1, static_cast<int>(steps));
    }

    void wave_lattice_tables(const Basis &basis, double *A, double *w)
    {
        const int n = basis.size();
        const QuadratureRule &gll = basis.quadrature();
        std::vector<double> x(n), D(static_cast<std::size_t>(n) * n);
        for (int i = 0; i < n; ++i)
        {
            x[i] = gll.x(i);
            w[i] = gll.w(i);
        }
        basis.deriv(n, x.data(), D.data()); // D[q + n j] = phi_j'(x_q)
        for (int k = 0; k < n; ++k)
            for (int j = 0; j < n; ++j)
            {
                double s = 0.0;
                for (int q = 0; q < n; ++q)
                    s += w[q] * D[q + n * k] * D[q + n * j];
                A[k * n + j] = s;
            }
    }
} // namespace cuddh
