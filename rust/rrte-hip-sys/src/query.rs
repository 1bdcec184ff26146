//! Ray queries (include/rrte_hip_query.h): closest hit, occlusion and pixel picking against a scene,
//! with the intersectors the frame kernel uses.  The engine-side use is selecting the object under
//! the mouse (crates/rrte-core/src/camera.rs:85-101 keeps `screen_to_ray` for it), line-of-sight
//! tests and placement probes.
//!
//! Mirrors include/rrte_hip_query.h the way lib.rs mirrors include/rrte_hip.h: `#[repr(C)]` records
//! in the header's field order, its constants, every entry point, and the safe `Context::raycast` /
//! `Context::pick` wrappers.  tests/test_query_abi.py checks this file mechanically against the
//! header (no cargo in the build image).
use crate::safe::{Context, Error, SceneIr};
use crate::*;

pub const RRTE_QUERY_CLOSEST: u32 = 0;
pub const RRTE_QUERY_ANY: u32 = 1;

/// One query ray.  The direction need not be unit length (normalised as Ray::new does, ray.rs:13-18);
/// t is measured along the normalised direction; `t_max` may be +inf.
#[repr(C)] #[derive(Clone, Copy, Debug, PartialEq)]
pub struct rrte_ray { pub origin: [f32; 3], pub t_min: f32, pub direction: [f32; 3], pub t_max: f32 }

/// One answer: `prim` = -1 (and `t` = +inf for a closest-hit query) on a miss.
#[repr(C)] #[derive(Clone, Copy, Debug, PartialEq)]
pub struct rrte_ray_hit { pub t: f32, pub prim: i32, pub point: [f32; 3], pub normal: [f32; 3],
    pub front_face: u32, pub tri: u32, pub material: i32, pub _pad: u32 }

extern "C" {
    pub fn rrte_hip_raycast(ctx: *mut rrte_ctx, scene: *const rrte_scene_ir, rays: *const rrte_ray, n: u32,
                            flags: u32, hits_out: *mut rrte_ray_hit) -> rrte_status;
    pub fn rrte_hip_raycast_async(ctx: *mut rrte_ctx, scene: *const rrte_scene_ir, d_rays: *const c_void, n: u32,
                                  flags: u32, d_hits: *mut c_void, stream: *mut c_void) -> rrte_status;
    pub fn rrte_hip_pick(ctx: *mut rrte_ctx, scene: *const rrte_scene_ir, params: *const rrte_render_params,
                         xy: *const u32, n: u32, hits_out: *mut rrte_ray_hit) -> rrte_status;
}

const MISS: rrte_ray_hit = rrte_ray_hit { t: f32::INFINITY, prim: -1, point: [0.0; 3], normal: [0.0; 3],
    front_face: 0, tri: 0, material: -1, _pad: 0 };

impl Context {
    /// rrte_hip_raycast: the closest hit of every ray (ray_color's search, raytracer.rs:103-113, over
    /// the ray's own interval) or, with `any_hit`, the first object in list order that occludes it.
    pub fn raycast(&mut self, scene: &SceneIr, rays: &[rrte_ray], any_hit: bool) -> Result<Vec<rrte_ray_hit>, Error> {
        let mut hits = vec![MISS; rays.len()];
        let ir = scene.raw();
        let flags = if any_hit { RRTE_QUERY_ANY } else { RRTE_QUERY_CLOSEST };
        let st = unsafe { rrte_hip_raycast(self.ctx, &ir, rays.as_ptr(), rays.len() as u32, flags, hits.as_mut_ptr()) };
        self.check(st)?;
        Ok(hits)
    }

    /// rrte_hip_pick: the closest hit under each pixel (x, y) of the `params.width` x `params.height`
    /// frame seen by the scene's camera -- the frame's own pixel-centre primary ray.
    pub fn pick(&mut self, scene: &SceneIr, params: &rrte_render_params, pixels: &[(u32, u32)])
        -> Result<Vec<rrte_ray_hit>, Error> {
        let xy: Vec<u32> = pixels.iter().flat_map(|&(x, y)| [x, y]).collect();
        let mut hits = vec![MISS; pixels.len()];
        let ir = scene.raw();
        let st = unsafe { rrte_hip_pick(self.ctx, &ir, params, xy.as_ptr(), pixels.len() as u32, hits.as_mut_ptr()) };
        self.check(st)?;
        Ok(hits)
    }
}
