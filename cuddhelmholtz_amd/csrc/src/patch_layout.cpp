// Patch layout of the plan kernels: see kernels/patch_layout.hpp.  Plain C++: nothing here touches the device.
#include "patch_layout.hpp"

#include <algorithm>
#include <cstring>
#include <string>

#include "cuddh_hip.h"

namespace cuddh_k
{
    namespace
    {
        constexpr int invalid_value = 1, not_supported = 801; // hipErrorInvalidValue, hipErrorNotSupported

        inline uint32_t spread_bits(uint32_t v)
        {
            v &= 0xFFFF;
            v = (v | (v << 8)) & 0x00FF00FF;
            v = (v | (v << 4)) & 0x0F0F0F0F;
            v = (v | (v << 2)) & 0x33333333;
            v = (v | (v << 1)) & 0x55555555;
            return v;
        }

        // element order: Morton curve over the centroids
        std::vector<int> morton_order(int n_elem, const double *xy)
        {
            std::vector<int> perm(n_elem);
            for (int e = 0; e < n_elem; ++e)
                perm[e] = e;
            if (!xy)
                return perm;
            double lo[2] = {xy[0], xy[1]}, hi[2] = {xy[0], xy[1]};
            for (int e = 0; e < n_elem; ++e)
                for (int a = 0; a < 2; ++a)
                {
                    lo[a] = std::min(lo[a], xy[2 * e + a]);
                    hi[a] = std::max(hi[a], xy[2 * e + a]);
                }
            std::vector<uint64_t> key(n_elem);
            for (int e = 0; e < n_elem; ++e)
            {
                uint32_t c[2];
                for (int a = 0; a < 2; ++a)
                {
                    const double span = hi[a] - lo[a];
                    const double t = span > 0 ? (xy[2 * e + a] - lo[a]) / span : 0.0;
                    c[a] = static_cast<uint32_t>(std::min(65535.0, std::max(0.0, t * 65535.0 + 0.5)));
                }
                key[e] = (static_cast<uint64_t>(spread_bits(c[0]) | (spread_bits(c[1]) << 1)) << 32) | static_cast<uint32_t>(e);
            }
            std::sort(key.begin(), key.end());
            for (int e = 0; e < n_elem; ++e)
                perm[e] = static_cast<int>(key[e] & 0xFFFFFFFFu);
            return perm;
        }

        // Greedy colouring: the lowest colour none of the item's local dofs has seen yet; `used` holds, per local dof, the colours
        // taken so far.  -1 when all max_colours are taken.
        int next_colour(std::vector<uint32_t> &used, const int *local, int n)
        {
            uint32_t taken = 0;
            for (int k = 0; k < n; ++k)
                taken |= used[local[k]];
            int c = 0;
            while (c < PatchLayout::max_colours && (taken >> c & 1u))
                ++c;
            if (c == PatchLayout::max_colours)
                return -1;
            for (int k = 0; k < n; ++k)
                used[local[k]] |= 1u << c;
            return c;
        }

        // the plan-native vector ordering: owned dofs patch by patch, then the border dofs in shared_dof order
        void native_ordering(int ndof, const std::vector<int> &shared_index, PatchLayout &L)
        {
            const int n_patches = L.n_patches;
            L.own_off.assign(n_patches + 1, 0);
            for (int q = 0; q < n_patches; ++q)
                L.own_off[q + 1] = L.own_off[q] + L.own_count[q];
            const int n_owned = L.own_off[n_patches];
            int bstride = 1;
            for (int q = 0; q < n_patches; ++q)
                bstride = std::max(bstride, L.dof_off[q + 1] - L.dof_off[q] - L.own_count[q]);
            L.bpos.assign((size_t)n_patches * bstride, 0);
            L.bslot.assign((size_t)n_patches * bstride, 0);
            L.global_of_native.assign(ndof, -1);
            for (int q = 0; q < n_patches; ++q)
            {
                const int first = L.dof_off[q], n_border = L.dof_off[q + 1] - first - L.own_count[q];
                for (int i = 0; i < L.own_count[q]; ++i)
                    L.global_of_native[L.own_off[q] + i] = L.dof_list[first + i];
                // (no border dofs: the padding is never read -- clamped index 0, value 0 = a valid position)
                for (int t = 0; t < bstride && n_border > 0; ++t)
                {
                    const int i = first + L.own_count[q] + std::min(t, n_border - 1);
                    L.bpos[(size_t)q * bstride + t] = n_owned + shared_index[L.dof_list[i]];
                    L.bslot[(size_t)q * bstride + t] = -L.slot_of[i] - 1;
                }
            }
            for (int j = 0; j < L.n_shared; ++j)
                L.global_of_native[n_owned + j] = L.shared_dof[j];
            // a dof no element touches would break the permutation: such a space keeps the reference ordering only
            L.has_native = n_owned + L.n_shared == ndof && std::find(L.global_of_native.begin(), L.global_of_native.end(), -1) == L.global_of_native.end();
            if (L.has_native)
            {
                L.n_owned = n_owned;
                L.bstride = bstride;
            }
            else
            {
                L.own_off.clear();
                L.bpos.clear();
                L.bslot.clear();
                L.global_of_native.clear();
            }
        }
    } // namespace

    int build_patch_layout(const PatchLayoutInput &in, PatchLayout &L)
    {
        L = PatchLayout{};
        const int ndof = in.ndof, n_elem = in.n_elem, nb = in.nb, nn = nb * nb, pe = in.pe, n_faces = in.n_faces;
        const std::vector<int> perm = morton_order(n_elem, in.xy);
        const int n_patches = (n_elem + pe - 1) / pe;
        L.pe = pe;
        L.n_patches = n_patches;
        L.perm.assign((size_t)n_patches * pe, -1);
        std::copy(perm.begin(), perm.end(), L.perm.begin());
        std::vector<int> patch_of_elem(n_elem);
        for (int pos = 0; pos < n_elem; ++pos)
            patch_of_elem[perm[pos]] = pos / pe;

        // ---- faces bucketed by the patch of their element
        L.face_off.assign(n_patches + 1, 0);
        for (int f = 0; f < n_faces; ++f)
            L.face_off[patch_of_elem[in.face_elem[f]] + 1]++;
        for (int q = 0; q < n_patches; ++q)
            L.face_off[q + 1] += L.face_off[q];
        L.face_id.resize(n_faces);
        {
            std::vector<int> cursor(L.face_off.begin(), L.face_off.end() - 1);
            for (int f = 0; f < n_faces; ++f)
                L.face_id[cursor[patch_of_elem[in.face_elem[f]]]++] = f;
        }

        // ---- how many patches touch a dof (a dof touched by one patch is OWNED by it: its result goes straight to y)
        std::vector<int> stamp(ndof, -1), loc(ndof, 0), touches(ndof, 0);
        for (int pos = 0; pos < n_elem; ++pos)
        {
            const int *gi = in.I + (size_t)nn * perm[pos];
            for (int n = 0; n < nn; ++n)
                if (stamp[gi[n]] != pos / pe)
                {
                    stamp[gi[n]] = pos / pe;
                    touches[gi[n]]++;
                }
        }
        std::fill(stamp.begin(), stamp.end(), -1);

        // ---- patch-local numbering and colours.  The owned dofs come first, the border dofs last: the write-out of an owned dof
        // then needs no destination entry -- it is the gather index -- so a kernel that knows own_count reads only the tail of
        // the patch's slot_of segment (helm_lane_kernel does).
        const int np2 = (nn + 1) / 2;
        L.dof_off.assign(n_patches + 1, 0);
        L.dof_list.reserve((size_t)n_elem * nn / 2);
        L.patch_nel.resize(n_patches);
        L.own_count.resize(n_patches);
        L.lidx.assign((size_t)n_patches * np2 * pe, 0);
        L.face_lidx.assign((size_t)n_faces * nb, 0);
        L.colour.assign((size_t)n_patches * pe, 0);
        L.face_col.assign(n_faces, 0);
        L.ncol = 1;
        int nfcol = 1;
        std::vector<int> border_first, local(std::max(nn, nb));
        std::vector<uint32_t> used;
        for (int q = 0; q < n_patches; ++q)
        {
            const int first = static_cast<int>(L.dof_list.size());
            L.dof_off[q] = first;
            const int nel = std::min(pe, n_elem - q * pe);
            L.patch_nel[q] = nel;
            border_first.clear();
            for (int le = 0; le < nel; ++le)
            {
                const int *gi = in.I + (size_t)nn * perm[q * pe + le];
                for (int n = 0; n < nn; ++n)
                {
                    const int g = gi[n];
                    if (stamp[g] == q)
                        continue;
                    stamp[g] = q;
                    if (touches[g] > 1)
                        border_first.push_back(g);
                    else
                    {
                        loc[g] = static_cast<int>(L.dof_list.size()) - first;
                        L.dof_list.push_back(g);
                    }
                }
            }
            L.own_count[q] = static_cast<int>(L.dof_list.size()) - first;
            for (const int g : border_first)
            {
                loc[g] = static_cast<int>(L.dof_list.size()) - first;
                L.dof_list.push_back(g);
            }
            const int nloc = static_cast<int>(L.dof_list.size()) - first;
            if (nloc > 65535) // lidx and face_lidx hold 16-bit local indices
                return invalid_value;
            L.max_loc = std::max(L.max_loc, nloc);

            used.assign(nloc, 0);
            for (int le = 0; le < nel; ++le)
            {
                const int *gi = in.I + (size_t)nn * perm[q * pe + le];
                for (int n = 0; n < nn; ++n)
                {
                    local[n] = loc[gi[n]];
                    L.lidx[((size_t)q * np2 + n / 2) * pe + le] |= static_cast<uint32_t>(local[n]) << (16 * (n & 1));
                }
                const int c = next_colour(used, local.data(), nn);
                if (c < 0)
                    return not_supported;
                L.colour[(size_t)q * pe + le] = static_cast<uint8_t>(c);
                L.ncol = std::max(L.ncol, c + 1);
            }
            used.assign(nloc, 0);
            for (int t = L.face_off[q]; t < L.face_off[q + 1]; ++t)
            {
                const int *fg = in.fI + (size_t)nb * L.face_id[t];
                for (int k = 0; k < nb; ++k)
                {
                    if (stamp[fg[k]] != q)
                        return invalid_value; // face dof not in its element's patch
                    local[k] = loc[fg[k]];
                    L.face_lidx[(size_t)t * nb + k] = static_cast<uint16_t>(local[k]);
                }
                const int c = next_colour(used, local.data(), nb);
                if (c < 0)
                    return not_supported;
                L.face_col[t] = static_cast<uint8_t>(c);
                nfcol = std::max(nfcol, c + 1);
            }
        }
        L.dof_off[n_patches] = static_cast<int>(L.dof_list.size());
        L.nfcol = n_faces > 0 ? nfcol : 0;

        // ---- dofs touched by more than one patch get one slot per touching patch
        std::vector<int> shared_index(ndof, -1);
        L.shared_off.assign(1, 0);
        for (int g = 0; g < ndof; ++g)
            if (touches[g] > 1)
            {
                shared_index[g] = static_cast<int>(L.shared_dof.size());
                L.shared_dof.push_back(g);
                L.shared_off.push_back(L.shared_off.back() + touches[g]);
            }
        L.n_shared = static_cast<int>(L.shared_dof.size());
        L.n_slots = L.shared_off.back();
        L.slot_of.resize(L.dof_list.size());
        {
            std::vector<int> fill(L.shared_off.begin(), L.shared_off.end() - 1);
            for (size_t i = 0; i < L.dof_list.size(); ++i)
            {
                const int j = shared_index[L.dof_list[i]];
                // owned: the global dof itself; border: -(slot) - 1, the slots of one dof being contiguous and ordered by patch
                L.slot_of[i] = j >= 0 ? -(fill[j]++) - 1 : L.dof_list[i];
            }
        }

        if (in.fused)
            native_ordering(ndof, shared_index, L);

        // ---- what the byte figures count
        L.list_entries = L.dof_list.size();
        const int rows[3] = {0, 64, 128};
        for (int k = 1; k < 3; ++k)
            L.dest_entries[k] = n_patches; // own_count
        L.dest_entries[0] = L.list_entries;
        for (int q = 0; q < n_patches; ++q)
        {
            const int nloc = L.dof_off[q + 1] - L.dof_off[q];
            L.owned_entries += L.own_count[q];
            L.native_list_entries += nloc - L.own_count[q];
            for (int k = 1; k < 3; ++k)
                L.dest_entries[k] += nloc - (L.own_count[q] / rows[k]) * rows[k];
        }

        // ---- fixed stride for the per-patch lists: segment q starts at q * max_loc and is padded with its last entry, so a kernel
        // can request its first indices without waiting for dof_off -- one dependent (scalar) round trip less at the head of every
        // wavefront's chain
        if (in.fixed_stride)
        {
            const int max_loc = L.max_loc;
            std::vector<int> dl((size_t)n_patches * max_loc), so((size_t)n_patches * max_loc);
            for (int q = 0; q < n_patches; ++q)
            {
                const int n = L.dof_off[q + 1] - L.dof_off[q];
                for (int i = 0; i < max_loc; ++i)
                {
                    dl[(size_t)q * max_loc + i] = L.dof_list[L.dof_off[q] + std::min(i, n - 1)];
                    so[(size_t)q * max_loc + i] = L.slot_of[L.dof_off[q] + std::min(i, n - 1)];
                }
            }
            L.dof_stride = max_loc;
            L.dof_list.swap(dl);
            L.slot_of.swap(so);
        }
        return 0;
    }
} // namespace cuddh_k

// ---- the layout alone, from raw arrays (tests)
struct cuddh_patch_layout
{
    cuddh_k::PatchLayout L;
};

namespace
{
    template <typename T>
    long long copy_out(const std::vector<T> &v, void *out, int count_only)
    {
        if (!count_only && out && !v.empty())
            std::memcpy(out, v.data(), v.size() * sizeof(T));
        return static_cast<long long>(v.size());
    }
    long long copy_out(long long v, void *out, int count_only) { return copy_out(std::vector<long long>(1, v), out, count_only); }
} // namespace

extern "C"
{
    int cuddh_patch_layout_create(cuddh_patch_layout **out, int ndof, int n_elem, int nb, const int *h_I, const double *h_xy, int n_faces,
                                  const int *h_fI, const int *h_face_elem, int pe, int fused, int fixed_stride)
    {
        *out = nullptr;
        if (ndof <= 0 || n_elem <= 0 || nb <= 0 || pe <= 0 || n_faces < 0 || !h_I || (n_faces > 0 && (!h_fI || !h_face_elem)))
            return 1;
        cuddh_k::PatchLayoutInput in;
        in.ndof = ndof;
        in.n_elem = n_elem;
        in.nb = nb;
        in.I = h_I;
        in.xy = h_xy;
        in.n_faces = n_faces;
        in.fI = h_fI;
        in.face_elem = h_face_elem;
        in.pe = pe;
        in.fused = fused != 0;
        in.fixed_stride = fixed_stride != 0;
        cuddh_patch_layout *h = new cuddh_patch_layout;
        const int err = cuddh_k::build_patch_layout(in, h->L);
        if (err)
            delete h;
        else
            *out = h;
        return err;
    }

    long long cuddh_patch_layout_array(const cuddh_patch_layout *h, const char *name_, void *out, int count_only)
    {
        if (!h || !name_)
            return -1;
        const cuddh_k::PatchLayout &L = h->L;
        const std::string name = name_;
#define CUDDH_LAYOUT_FIELD(field) \
    if (name == #field)           \
        return copy_out(L.field, out, count_only);
        CUDDH_LAYOUT_FIELD(perm)
        CUDDH_LAYOUT_FIELD(dof_off)
        CUDDH_LAYOUT_FIELD(dof_list)
        CUDDH_LAYOUT_FIELD(slot_of)
        CUDDH_LAYOUT_FIELD(own_count)
        CUDDH_LAYOUT_FIELD(patch_nel)
        CUDDH_LAYOUT_FIELD(lidx)
        CUDDH_LAYOUT_FIELD(colour)
        CUDDH_LAYOUT_FIELD(face_off)
        CUDDH_LAYOUT_FIELD(face_id)
        CUDDH_LAYOUT_FIELD(face_lidx)
        CUDDH_LAYOUT_FIELD(face_col)
        CUDDH_LAYOUT_FIELD(shared_dof)
        CUDDH_LAYOUT_FIELD(shared_off)
        CUDDH_LAYOUT_FIELD(own_off)
        CUDDH_LAYOUT_FIELD(bpos)
        CUDDH_LAYOUT_FIELD(bslot)
        CUDDH_LAYOUT_FIELD(global_of_native)
        CUDDH_LAYOUT_FIELD(pe)
        CUDDH_LAYOUT_FIELD(n_patches)
        CUDDH_LAYOUT_FIELD(dof_stride)
        CUDDH_LAYOUT_FIELD(max_loc)
        CUDDH_LAYOUT_FIELD(ncol)
        CUDDH_LAYOUT_FIELD(nfcol)
        CUDDH_LAYOUT_FIELD(n_shared)
        CUDDH_LAYOUT_FIELD(n_slots)
        CUDDH_LAYOUT_FIELD(has_native)
        CUDDH_LAYOUT_FIELD(n_owned)
        CUDDH_LAYOUT_FIELD(bstride)
        CUDDH_LAYOUT_FIELD(list_entries)
        CUDDH_LAYOUT_FIELD(owned_entries)
        CUDDH_LAYOUT_FIELD(native_list_entries)
#undef CUDDH_LAYOUT_FIELD
        if (name == "dest_entries")
            return copy_out(std::vector<long long>(L.dest_entries, L.dest_entries + 3), out, count_only);
        return -1;
    }

    void cuddh_patch_layout_destroy(cuddh_patch_layout *h) { delete h; }
}
