// The persistent voxel map as its two translation units see it: voxel_map.hip (insert, extract, retain: everything
// that changes the table) and voxel_map_icp.hip (nearest and frame-to-map ICP: the table is only read).
#pragma once
#include "solo_icp.hpp"
#include "voxel_grid.hpp"

struct a3d_voxel_map {
  a3d_context* ctx = nullptr;
  a3d::VoxelGrid grid{};
  bool with_normals = false, with_colors = false;
  uint64_t reserve_cells = 0;
  // the device block of the current table (null until the first insert that holds a point)
  void* block = nullptr;
  size_t block_bytes = 0;
  uint64_t slots = 0;
  a3d::VoxelSlot* table = nullptr;
  float* points = nullptr;
  float* normals = nullptr;
  uint32_t* colors = nullptr;  // [slots] r | g << 8 | b << 16, or null
  unsigned long long* cell_count = nullptr;
  // a map of means (a3d_voxel_map_new_mean) keeps per slot, beside the row: the count of the cell's points, the sums of
  // their lattice offsets, of their rounded normals (maps with normals) and of their colours (maps with colours), and
  // the number of the last insert call that touched the cell; all null in a nearest-point map
  bool mean = false;
  unsigned long long* sum_n = nullptr;  // [slots]
  long long* sum_s = nullptr;           // [slots][3]
  long long* sum_t = nullptr;           // [slots][3] or null
  unsigned long long* sum_c = nullptr;  // [slots][3] or null
  uint32_t* epoch = nullptr;            // [slots]
  uint32_t epoch_no = 0;                // of the last insert call that launched
  uint64_t cells = 0, total = 0, dropped_total = 0, growths = 0;
  // the working state of the frame-to-map ICP (voxel_map_icp.hip): taken by the first align or accumulate and released
  // with the map (solo_icp_release)
  a3d::SoloIcp icp;
};
