//! Frame AOVs (include/rrte_hip_aov.h): per-pixel depth, object and material ids, triangle index,
//! normal, position and albedo of a view or a rectangle of it -- the id buffer of selection
//! outlines, the depth gizmos are composited against, the guides of a denoiser.  Every value is the
//! field of the `rrte_ray_hit` that `Context::pick` returns for that pixel.
//!
//! Mirrors include/rrte_hip_aov.h the way query.rs mirrors include/rrte_hip_query.h: `#[repr(C)]`
//! records in the header's field order, its constants, every entry point, and the safe
//! `Context::render_aov` wrapper.  tests/test_aov_abi.py checks this file mechanically against the
//! header (no cargo in the build image).
use crate::safe::{Context, Error, SceneIr};
use crate::*;

pub const RRTE_AOV_DEPTH: u32 = 1;
pub const RRTE_AOV_PRIM: u32 = 2;
pub const RRTE_AOV_MATERIAL: u32 = 4;
pub const RRTE_AOV_TRI: u32 = 8;
pub const RRTE_AOV_NORMAL: u32 = 16;
pub const RRTE_AOV_POSITION: u32 = 32;
pub const RRTE_AOV_ALBEDO: u32 = 64;
pub const RRTE_AOV_ALL: u32 = 127;

/// What to compute: the planes and the rectangle of the frame (all zero: the whole frame).
#[repr(C)] #[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct rrte_aov_desc { pub planes: u32, pub x0: u32, pub y0: u32, pub width: u32, pub height: u32,
    pub _pad: [u32; 3] }

/// Where each plane goes (row-major over the rectangle, tightly packed); only the pointers of
/// requested planes are read.
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct rrte_aov_buffers { pub depth: *mut f32, pub prim: *mut i32, pub material: *mut i32, pub tri: *mut u32,
    pub normal: *mut f32, pub position: *mut f32, pub albedo: *mut f32, pub _reserved: *mut c_void }

extern "C" {
    pub fn rrte_hip_render_aov(ctx: *mut rrte_ctx, scene: *const rrte_scene_ir, params: *const rrte_render_params,
                               desc: *const rrte_aov_desc, out: *const rrte_aov_buffers) -> rrte_status;
    pub fn rrte_hip_render_aov_async(ctx: *mut rrte_ctx, scene: *const rrte_scene_ir,
                                     params: *const rrte_render_params, desc: *const rrte_aov_desc,
                                     d_out: *const rrte_aov_buffers, stream: *mut c_void) -> rrte_status;
}

/// The planes of one call; a plane that was not requested is empty.  `normal`, `position` and
/// `albedo` hold four floats per pixel.
#[derive(Clone, Debug, Default)]
pub struct AovPlanes {
    pub width: u32,
    pub height: u32,
    pub depth: Vec<f32>,
    pub prim: Vec<i32>,
    pub material: Vec<i32>,
    pub tri: Vec<u32>,
    pub normal: Vec<f32>,
    pub position: Vec<f32>,
    pub albedo: Vec<f32>,
}

impl Context {
    /// rrte_hip_render_aov: the planes `planes` (RRTE_AOV_*) of the rectangle `rect` = (x0, y0, width,
    /// height) of the `params.width` x `params.height` frame seen by the scene's camera (None, or
    /// all zero as in the header: the whole frame).
    pub fn render_aov(&mut self, scene: &SceneIr, params: &rrte_render_params, planes: u32,
                      rect: Option<(u32, u32, u32, u32)>) -> Result<AovPlanes, Error> {
        let (x0, y0, width, height) = rect.unwrap_or((0, 0, 0, 0));
        let desc = rrte_aov_desc { planes, x0, y0, width, height, _pad: [0; 3] };
        // the vectors are sized as the library reads the desc: an all-zero rectangle is the whole frame
        let whole = (x0 | y0 | width | height) == 0;
        let (w, h) = if whole { (params.width, params.height) } else { (width, height) };
        let n = w as usize * h as usize;
        let len = |bit: u32, per: usize| if planes & bit != 0 { n * per } else { 0 };
        let mut out = AovPlanes { width: w, height: h, depth: vec![0.0; len(RRTE_AOV_DEPTH, 1)],
            prim: vec![0; len(RRTE_AOV_PRIM, 1)], material: vec![0; len(RRTE_AOV_MATERIAL, 1)],
            tri: vec![0; len(RRTE_AOV_TRI, 1)], normal: vec![0.0; len(RRTE_AOV_NORMAL, 4)],
            position: vec![0.0; len(RRTE_AOV_POSITION, 4)], albedo: vec![0.0; len(RRTE_AOV_ALBEDO, 4)] };
        let bufs = rrte_aov_buffers { depth: out.depth.as_mut_ptr(), prim: out.prim.as_mut_ptr(),
            material: out.material.as_mut_ptr(), tri: out.tri.as_mut_ptr(), normal: out.normal.as_mut_ptr(),
            position: out.position.as_mut_ptr(), albedo: out.albedo.as_mut_ptr(), _reserved: std::ptr::null_mut() };
        let ir = scene.raw();
        let st = unsafe { rrte_hip_render_aov(self.ctx, &ir, params, &desc, &bufs) };
        self.check(st)?;
        Ok(out)
    }
}
