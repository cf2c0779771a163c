// Patch layout of the plan kernels (helmholtz_fused.hip): which elements form a patch, the patch-local dof numbering, the
// colours, the slots of the patch-border dofs and the plan-native vector ordering.  Host-only integer combinatorics
// (src/patch_layout.cpp, no HIP): plan creation uploads the arrays as they are, and tests read them through
// cuddh_patch_layout_* (include/cuddh_hip.h) without a GPU.  DESIGN.md 4.1, "Patch layout".
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace cuddh_k
{
    struct PatchLayoutInput
    {
        int ndof = 0, n_elem = 0, nb = 0;
        const int *I = nullptr;     // (nb, nb, n_elem) element node -> global dof
        const double *xy = nullptr; // (2, n_elem) element centroids, or null: keep the element order
        int n_faces = 0;
        const int *fI = nullptr;        // (nb, n_faces) face node -> global dof
        const int *face_elem = nullptr; // (n_faces) the element each face belongs to
        int pe = 32;                    // elements per patch
        bool fused = false;             // complex Helmholtz plan: also gets the plan-native vector ordering
        bool fixed_stride = false;      // dof_list / slot_of: one segment of max_loc entries per patch, padded with its last entry
    };

    struct PatchLayout
    {
        static constexpr int max_colours = 31; // per patch, for elements and for faces: a 32nd colour is refused (801), never shared

        int pe = 0, n_patches = 0;
        std::vector<int> perm; // [n_patches][pe] element at every patch position (Morton order of the centroids), -1 behind the last
        // per patch: owned dofs (touched by no other patch) first, border dofs last, each group in the order its dofs are first met
        std::vector<int> dof_off;   // [n_patches + 1] offsets into the PACKED lists (also kept when the lists are padded)
        std::vector<int> dof_list;  // global dof of every patch-local dof
        std::vector<int> slot_of;   // owned: the global dof itself; border: -(slot) - 1
        int dof_stride = 0;         // != 0: dof_list / slot_of hold max_loc entries per patch, padded with the patch's last entry
        std::vector<int> own_count; // [n_patches]
        std::vector<int> patch_nel; // [n_patches] elements in the patch (pe except possibly the last)
        std::vector<uint32_t> lidx; // [n_patches][ceil(nb*nb/2)][pe]: element nodes 2j, 2j+1 -> patch-local dofs, lo | hi << 16
        std::vector<uint8_t> colour; // [n_patches][pe]: elements of one colour in one patch share no dof
        // boundary faces, grouped by the patch of their element
        std::vector<int> face_off, face_id; // [n_patches + 1]; original face index at every grouped position
        std::vector<uint16_t> face_lidx;    // [n_faces][nb] patch-local dof of every face node
        std::vector<uint8_t> face_col;      // [n_faces]
        // border dof j (touched by several patches) owns the contiguous slots shared_off[j] .. shared_off[j+1], one per touching
        // patch in increasing patch order
        std::vector<int> shared_dof, shared_off;
        int max_loc = 0, ncol = 0, nfcol = 0, n_shared = 0, n_slots = 0;
        // plan-native vector ordering (fused plans in which every dof is touched by an element): [patch 0's owned dofs | patch 1's
        // | ... | border dofs in shared_dof order]
        bool has_native = false;
        int n_owned = 0, bstride = 0;
        std::vector<int> own_off;          // [n_patches + 1] prefix sum of own_count
        std::vector<int> bpos, bslot;      // [n_patches][bstride] native position and slot of the patch's border dofs, padded with the last
        std::vector<int> global_of_native; // [ndof]
        // what the byte figures count
        size_t list_entries = 0;        // patch-local dofs over all patches (the packed length of dof_list)
        size_t owned_entries = 0;       // of them owned
        size_t native_list_entries = 0; // border entries over all patches (bpos / bslot without the padding)
        // entries of slot_of a write-out reads when it skips whole rows of owned dofs: rows of 64, of 128, [0] no rows (all of it)
        size_t dest_entries[3] = {0, 0, 0};
        size_t dest_entries_for_row(int row) const { return dest_entries[row == 64 ? 1 : (row == 128 ? 2 : 0)]; }
    };

    // 0, or the hipError_t value plan creation returns: 1 (hipErrorInvalidValue) for more than 65,535 local dofs in a patch or a
    // face dof outside its element's patch, 801 (hipErrorNotSupported) when a patch needs more than max_colours colours
    int build_patch_layout(const PatchLayoutInput &in, PatchLayout &out);
} // namespace cuddh_k
