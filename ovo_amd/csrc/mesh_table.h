// mesh_table.h -- written by tools/gen_mesh_table.py, not by hand (tests/test_mesh_host.py compares).  Marching tetrahedra on the Kuhn
// triangulation: MESH_TABLE[n][m] for tetrahedron n under the inside-mask m.  Bits 0-1: the number of triangles; vertex v (0 .. 5) in bits
// 2 + 6 v .. 7 + 6 v: owner cube corner (x + 2 y + 4 z) | slot << 3.  MESH_TET_CORNERS[n]: the cube corners c0 .. c3, four bits each.
#pragma once
#include <stdint.h>

__device__ const uint64_t MESH_TABLE[6][16] = {
    {0x0000000000ull, 0x00000c1801ull, 0x0000026901ull, 0x09a58a7062ull, 0x000004c961ull, 0x13240c1302ull, 0x13a4061302ull, 0x000004e9c1ull, 0x00000a53c1ull, 0x294c04d802ull, 0x094c04f002ull, 0x0000025361ull, 0x29258c2962ull, 0x00000a4901ull, 0x0000063001ull, 0x0000000000ull},
    {0x0000000000ull, 0x0000083001ull, 0x00000a5101ull, 0x29460c2982ull, 0x0000044d81ull, 0x1134037002ull, 0x2934036002ull, 0x00000a4dc1ull, 0x00000369c1ull, 0x0da4080d02ull, 0x0d440c0d02ull, 0x0000035181ull, 0x11a60a7082ull, 0x0000046901ull, 0x00000c2001ull, 0x0000000000ull},
    {0x0000000000ull, 0x0000063021ull, 0x0000088221ull, 0x22098c2262ull, 0x0000009361ull, 0x024c84f022ull, 0x224c84d822ull, 0x00000893c1ull, 0x000004e2c1ull, 0x1388861322ull, 0x13088c1322ull, 0x000004c261ull, 0x028988b062ull, 0x000000a221ull, 0x00000c1821ull, 0x0000000000ull},
    {0x0000000000ull, 0x00000c2821ull, 0x000004a221ull, 0x128a88b0a2ull, 0x00000192a1ull, 0x06488c0622ull, 0x06888a0622ull, 0x000001a2c1ull, 0x00000886c1ull, 0x221881a822ull, 0x121881b022ull, 0x00000486a1ull, 0x224a8c22a2ull, 0x0000089221ull, 0x00000a3021ull, 0x0000000000ull},
    {0x0000000000ull, 0x00000c2041ull, 0x0000011c41ull, 0x0472073082ull, 0x0000034481ull, 0x0d110c0d42ull, 0x0d71080d42ull, 0x0000035cc1ull, 0x0000070dc1ull, 0x1c35036042ull, 0x0435037042ull, 0x0000010d81ull, 0x1c120c1c82ull, 0x0000070441ull, 0x0000083041ull, 0x0000000000ull},
    {0x0000000000ull, 0x00000a3041ull, 0x0000070c41ull, 0x1c328c1ca2ull, 0x00000306a1ull, 0x0c1901b042ull, 0x1c1901a842ull, 0x00000706c1ull, 0x0000019cc1ull, 0x06710a0642ull, 0x06310c0642ull, 0x0000018ca1ull, 0x0c728730a2ull, 0x0000031c41ull, 0x00000c2841ull, 0x0000000000ull},
};
constexpr uint32_t MESH_TET_CORNERS[6] = {0x7310, 0x7510, 0x7320, 0x7620, 0x7540, 0x7640};
