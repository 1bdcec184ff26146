//! Deforming meshes: device-side BVH refit (include/rrte_hip_refit.h).
//!
//! `rrte_hip_mesh_refit` tells the context that a scene's mesh arrays are a deformation (same counts,
//! same index values) of the ones its mesh data was built or last refitted from; the next render or
//! query of that scene refits the BVHs on the device instead of building them on the host.
//! `rrte_hip_refit_info` counts what happened; `rrte_hip_mesh_nodes` and `rrte_hip_mesh_slots` are
//! diagnostic read-backs.  Mirrors the header the way mesh.rs mirrors include/rrte_hip_mesh.h;
//! tests/test_refit_abi.py checks this file mechanically against the header (no cargo in the build
//! image).
use crate::safe::{Context, Error};
use crate::*;

/// Refit counters of a context.
#[repr(C)] #[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct rrte_refit_info { pub refits: u64, pub device_refits: u64, pub levels: u32, pub deformed: u32 }

extern "C" {
    pub fn rrte_hip_mesh_refit(ctx: *mut rrte_ctx, scene: *const rrte_scene_ir) -> rrte_status;
    pub fn rrte_hip_refit_info(ctx: *mut rrte_ctx, out: *mut rrte_refit_info) -> rrte_status;
    pub fn rrte_hip_mesh_nodes(ctx: *mut rrte_ctx, out: *mut c_void, bytes: usize, records: *mut u32) -> rrte_status;
    pub fn rrte_hip_mesh_slots(ctx: *mut rrte_ctx, out: *mut u32, count: usize, slots: *mut u32) -> rrte_status;
}

impl Context {
    /// rrte_hip_mesh_refit: `scene`'s mesh arrays deform the ones the context's mesh data came from.
    /// Host only.  `Err` with RRTE_INVALID_ARG when refused (the context is as it was: render plainly).
    ///
    /// # Safety
    /// `scene`'s pointers must be valid for its counts.
    pub unsafe fn mesh_refit(&mut self, scene: &rrte_scene_ir) -> Result<(), Error> {
        let st = rrte_hip_mesh_refit(self.ctx, scene);
        self.check(st)
    }

    /// rrte_hip_refit_info.  Host only.
    pub fn refit_info(&mut self) -> Result<rrte_refit_info, Error> {
        let mut info = rrte_refit_info::default();
        let st = unsafe { rrte_hip_refit_info(self.ctx, &mut info) };
        self.check(st)?;
        Ok(info)
    }

    /// rrte_hip_mesh_nodes: the current scene version's BVH interior records, 16 f32 each.
    pub fn mesh_nodes(&mut self) -> Result<Vec<[f32; 16]>, Error> {
        let mut n = 0u32;
        let st = unsafe { rrte_hip_mesh_nodes(self.ctx, std::ptr::null_mut(), 0, &mut n) };
        self.check(st)?;
        let mut out = vec![[0f32; 16]; n as usize];
        let st = unsafe { rrte_hip_mesh_nodes(self.ctx, out.as_mut_ptr() as *mut c_void, out.len() * 64, &mut n) };
        self.check(st)?;
        Ok(out)
    }

    /// rrte_hip_mesh_slots: per device triangle slot, its triangle's index within its range.
    pub fn mesh_slots(&mut self) -> Result<Vec<u32>, Error> {
        let mut n = 0u32;
        let st = unsafe { rrte_hip_mesh_slots(self.ctx, std::ptr::null_mut(), 0, &mut n) };
        self.check(st)?;
        let mut out = vec![0u32; n as usize];
        let st = unsafe { rrte_hip_mesh_slots(self.ctx, out.as_mut_ptr(), out.len(), &mut n) };
        self.check(st)?;
        Ok(out)
    }
}
