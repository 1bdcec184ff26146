//! Mesh instances and mesh sharing diagnostics (include/rrte_hip_mesh.h).
//!
//! `RRTE_PRIM_MESH_INSTANCE` is the prim kind of a triangle range placed in the world through the
//! prim's `trs` (include/rrte_hip.h spells out its arithmetic); `rrte_hip_mesh_info` reports how the
//! context stores the ranges: once per distinct range, and rebuilt only when the mesh arrays or the
//! set of ranges change.  Mirrors the header the way query.rs mirrors include/rrte_hip_query.h;
//! tests/test_mesh_abi.py checks this file mechanically against the header (no cargo in the build
//! image).  Lowering engine mesh entities to instances lives with the renderer crate, not here.
use crate::safe::{Context, Error};
use crate::*;

pub const RRTE_PRIM_MESH_INSTANCE: u32 = 9;

/// How the context stores the current scene's triangle ranges.
#[repr(C)] #[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct rrte_mesh_info { pub bvh_builds: u64, pub ranges: u32, pub tri_slots: u32, pub bvh_nodes: u32,
    pub _pad: u32 }

extern "C" {
    pub fn rrte_hip_mesh_info(ctx: *mut rrte_ctx, out: *mut rrte_mesh_info) -> rrte_status;
}

impl Context {
    /// rrte_hip_mesh_info: BVH builds so far and the ranges, triangle slots and BVH records of the
    /// scene the context holds.  Host only.
    pub fn mesh_info(&mut self) -> Result<rrte_mesh_info, Error> {
        let mut info = rrte_mesh_info::default();
        let st = unsafe { rrte_hip_mesh_info(self.ctx, &mut info) };
        self.check(st)?;
        Ok(info)
    }
}
