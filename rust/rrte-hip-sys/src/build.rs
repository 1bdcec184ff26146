//! The mesh build policy: device-side BVH build (include/rrte_hip_build.h).
//!
//! `rrte_hip_set_mesh_build` chooses who builds the BVH of a new mesh or a changed topology at the
//! next mesh-cache miss: the host's binned-SAH builder (the default) or the LBVH kernels on the
//! context's upload stream.  `rrte_hip_build_info` counts what happened.  Mirrors the header the way
//! refit.rs mirrors include/rrte_hip_refit.h; tests/test_build_abi.py checks this file mechanically
//! against the header (no cargo in the build image).
use crate::safe::{Context, Error};
use crate::*;

pub const RRTE_MESH_BUILD_HOST: u32 = 0;
pub const RRTE_MESH_BUILD_DEVICE: u32 = 1;

/// Build counters of a context.
#[repr(C)] #[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct rrte_build_info { pub device_builds: u64, pub host_fallbacks: u64, pub policy: u32, pub depth: u32 }

extern "C" {
    pub fn rrte_hip_set_mesh_build(ctx: *mut rrte_ctx, policy: u32) -> rrte_status;
    pub fn rrte_hip_build_info(ctx: *mut rrte_ctx, out: *mut rrte_build_info) -> rrte_status;
}

impl Context {
    /// rrte_hip_set_mesh_build: `RRTE_MESH_BUILD_HOST` or `RRTE_MESH_BUILD_DEVICE`.  Host only; takes
    /// effect at the next mesh-cache miss and rebuilds nothing by itself.
    pub fn set_mesh_build(&mut self, policy: u32) -> Result<(), Error> {
        let st = unsafe { rrte_hip_set_mesh_build(self.ctx, policy) };
        self.check(st)
    }

    /// rrte_hip_build_info.  Host only.
    pub fn build_info(&mut self) -> Result<rrte_build_info, Error> {
        let mut info = rrte_build_info::default();
        let st = unsafe { rrte_hip_build_info(self.ctx, &mut info) };
        self.check(st)?;
        Ok(info)
    }
}
