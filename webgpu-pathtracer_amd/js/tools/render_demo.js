'use strict';
// Headless equivalent of the reference's main loop (src/main.ts:374-400) on the default
// scene: N calls of renderer.render(scene, camera), then read-back.
//   node render_demo.js --env env.f32 --width 64 --height 64 --frames 3 --bounces 4 --out prefix
//   --hdr file.hdr     a Radiance map (1024x512) instead of raw float texels (main.ts:41-46)
//   --model file.glb   replace the default meshes by a loaded model (.glb/.gltf/.obj), main.ts:251-279
//   --devices 0,1,2    a device group: Renderer.create({ devices: [0, 1, 2] }) -- the same loop on several GPUs
//   --aovs             also the first-hit feature images: <prefix>_albedo.png, <prefix>_normal.png (0.5 n + 0.5) and
//                      <prefix>_position.f32 (raw RGBA float: position xyz, t; row 0 = bottom)
//   --guided           also the feature-guided de-noise of the final mean (renderer.denoiseGuided(), default parameters):
//                      <prefix>_guided.f32 (raw RGBA float; row 0 = bottom) and <prefix>_guided.png (the canvas drawn from it)
//   --guided-variance  the moments image on from the start, then renderer.denoiseGuided({ variance: true, present: true }): the outputs of
//                      --guided from the variance-guided filter, <prefix>_guided_variance.f32 (raw float, one per texel) and
//                      <prefix>_moments.f32 (raw RGBA float: M2.rgb, n).  Not together with --guided: both write <prefix>_guided.*
//   --young            with --guided-variance: denoiseGuided({ ..., young: true }) -- a texel with fewer than four samples (disoccluded by
//                      --reproject, or every texel of a one-frame view) takes its variance from the samples of its 7 x 7 neighbours
//   --despike          with --guided or --guided-variance: denoiseGuided({ ..., despike: true }) -- the firefly pre-pass ahead of the filter (a
//                      texel brighter than all 3 x 3 neighbours of its material and hit flag is scaled down to the brightest of them);
//                      prints the clamped share and lists the count under "despiked"
//   --until <rmse>     sample until converged instead of a fixed count: renderer.renderUntil(scene, camera, rmse, { maxFrames: --frames })
//                      with the moments image on; --min-frames N (16), --check-every N (the batch capacity), --no-lookahead.  Prints the
//                      frames taken and the summary of the estimate under "until"
//   --adaptive         with --until: renderUntil(..., { adaptive: true }) -- converged tiles stop being sampled (renderer.freezeConverged after every
//                      check); --guard 0|1 (1): keep a converged tile sampling while one of its eight neighbours is not.  "until" gains `sampled`;
//                      also writes <prefix>_mask.u8 (the final sample mask, one byte per 8 x 8 tile) and <prefix>_moments.f32
//   --orbit N          N views around the scene instead of one: the camera turns about the vertical axis through its target by --step DEG (2)
//                      per view and every view takes --spp K frames (4); writes <prefix>_view<i>.png, <prefix>_view<i>.acc.f32 and
//                      <prefix>_view<i>.uniforms.bin (the view's 96-byte raytrace uniform block: its camera) per view.
//                      Between views renderer.reset(), or with --reproject renderer.setMeanByCount(true) from the start and
//                      renderer.reproject(scene, camera) (the mean is carried across the move); with --guided-variance every view's PNG
//                      is drawn from renderer.denoiseGuided({ variance: true, present: true }).  The usual outputs are the last view's
//   --slide N          N steps of a moving object under a fixed camera: the demo's box slides by --step D (0.1) along x per step and every
//                      step takes --spp K frames (4); writes <prefix>_step<i>.png, <prefix>_step<i>.acc.f32 and <prefix>_step<i>.uniforms.bin per step.  Between steps
//                      scene.needsUpdate = true and renderer.reset(), or with --reproject renderer.setMeanByCount(true) from the start and
//                      renderer.reprojectScene(scene, camera) (the mean follows the box).  Not together with --orbit
//   --refit            with --slide: renderer.refit = true -- from the second step on the tree is not rebuilt on the host: the device re-fits
//                      the boxes of the uploaded tree to the moved triangles (mi3pt_device_refit_bvh).  Prints the cost ratio of the
//                      re-fitted tree over the last full build per step, lists them under "refit" (null: that step was built), and writes
//                      <prefix>_step<i>.nodes.bin, the 48-byte records the device holds in that step
//   --validate K       with --reproject in the --orbit and --slide loops: the carried mean is not merged at once but held, validated against the
//                      view's first K frames (K <= --spp) and then merged -- what reproject(scene, camera, { validate: K }) does, spelled out as
//                      holdHistory() / mergeHistory() around two moments reads (the held counts nh; the counts n' after the merge, n = K before
//                      it).  Prints the share of carried samples kept per view, sum(n' - n) / sum(nh), and lists it under "validate"
//   --device-bvh       Renderer.create({ deviceBvh: true }): the tree is built on the GPU from the uploaded triangles (csrc/pt_lbvh.hip)
//   --device-bvh=lbvh|ploc  the same by name: the linear BVH, or the locally-ordered clustering (csrc/pt_ploc.hip), with
//                      --device-bvh-radius=R (1 .. 64, default 16)
//   --second-scene     after the loop: remove the scene's last mesh (the sphere of the default scene), mark the scene changed,
//                      reset and run the loop again -- a second updateScene with another triangle count; the outputs are the
//                      second scene's
// Writes <prefix>.acc.f32 (accumulation, RGBA float), <prefix>.canvas.rgba8 and prints a
// JSON summary.  Needs a HIP device.
const fs = require('fs');
const pt = require('..');
const { buildDefaultScene, PARAMS } = require('../examples/default_scene');

function arg(name, dflt) {
  const i = process.argv.indexOf('--' + name);
  return i >= 0 ? process.argv[i + 1] : dflt;
}

async function main() {
  const guidedVariance = process.argv.includes('--guided-variance');
  if (guidedVariance && process.argv.includes('--guided')) throw new Error('--guided and --guided-variance both write <prefix>_guided.f32 / .png: give one of them');
  const young = process.argv.includes('--young');
  if (young && !guidedVariance) throw new Error('--young changes the variance-guided filter: give --guided-variance too');
  const despike = process.argv.includes('--despike');
  if (despike && !guidedVariance && !process.argv.includes('--guided')) throw new Error('--despike runs ahead of the guided filter: give --guided or --guided-variance too');
  let despiked;
  const sayDespiked = () => {
    despiked = renderer.readGuidedDespiked();
    console.error('despike: ' + despiked + ' of ' + width * height + ' texels clamped (' + (100 * despiked / (width * height)).toFixed(2) + ' %)');
  };
  const width = parseInt(arg('width', '256'), 10), height = parseInt(arg('height', '256'), 10);
  const frames = parseInt(arg('frames', '4'), 10), bounces = parseInt(arg('bounces', String(PARAMS.maxBounces)), 10);
  const envPath = arg('env', null), out = arg('out', 'demo');
  let envData = null;
  if (envPath) {
    const b = fs.readFileSync(envPath);
    envData = new Float32Array(b.buffer, b.byteOffset, b.length / 4);
  }
  const diag = await pt.Renderer.diagnostic();
  if (!diag.supported) throw new Error('HIP device not found.');
  const devices = arg('devices', null);
  const options = { enableTimestampQuery: true };
  if (devices) options.devices = devices.split(',').map((d) => parseInt(d, 10));
  if (process.argv.includes('--device-bvh')) options.deviceBvh = true;
  for (const a of process.argv) {
    if (a.startsWith('--device-bvh=')) options.deviceBvh = a.slice('--device-bvh='.length);
    if (a.startsWith('--device-bvh-radius=')) options.deviceBvhRadius = parseInt(a.slice('--device-bvh-radius='.length), 10);
  }
  const renderer = await pt.Renderer.create(options);
  const { scene, camera } = buildDefaultScene(envData);
  if (arg('hdr', null)) scene.environment = new pt.RGBELoader().setDataType(pt.FloatType).load(arg('hdr'));
  const modelPath = arg('model', null);
  if (modelPath) {
    const model = /\.obj$/i.test(modelPath) ? new pt.OBJLoader().load(modelPath) : new pt.GLTFLoader().load(modelPath).scene;
    pt.placeModel(model);
    scene.clear();
    scene.add(model);
    scene.needsUpdate = true;
  }
  const events = [];
  for (const ev of ['start', 'reset', 'progress', 'complete', 'resize']) renderer.on(ev, () => events.push(ev));
  renderer.frames = frames;
  renderer.scalingFactor = parseFloat(arg('scale', '1'));
  renderer.setUniforms('raytrace', { maxBounces: bounces, envMapIntensity: PARAMS.envMapIntensity });
  renderer.setUniforms('accumulate', { enabled: PARAMS.accumulate ? 1 : 0 });
  renderer.setUniforms('fullscreen', { denoise: PARAMS.denoise ? 1 : 0, tonemapping: PARAMS.tonemapping });
  const untilArg = arg('until', null);
  if (guidedVariance || untilArg !== null) renderer.setMoments(true);
  const orbit = parseInt(arg('orbit', '0'), 10), reproject = process.argv.includes('--reproject');
  const slide = parseInt(arg('slide', '0'), 10);
  const refit = process.argv.includes('--refit'), refitRatios = [];
  if (refit && !(slide > 0)) throw new Error('--refit re-fits the tree between the steps of --slide: give --slide N too');
  if (refit) renderer.refit = true;
  const validate = parseInt(arg('validate', '0'), 10), keptShares = [];
  // after a reprojection that carried something: hold it and remember its counts
  const hold = (carried) => {
    if (!carried || !(validate > 0)) return null;
    const held = renderer.readMoments();
    renderer.holdHistory();
    return held;
  };
  // a view's frames; the held history is merged once K of them are in
  const sample = (spp, held, what) => {
    const k = Math.min(validate, spp);
    for (let i = 0; i < spp + 1; i++) {                                      // the last call only presents
      renderer.render(scene, camera);
      if (held && i + 1 === k) {
        renderer.mergeHistory();
        const now = renderer.readMoments();
        let kept = 0, carried = 0;
        for (let t = 3; t < now.length; t += 4) { kept += now[t] - k; carried += held[t]; }
        keptShares.push(carried > 0 ? kept / carried : 0);
        console.error('--validate ' + k + ': ' + what + ': ' + (100 * keptShares[keptShares.length - 1]).toFixed(1) + ' % of ' + carried + ' carried samples kept');
      }
    }
  };
  if (orbit > 0 && slide > 0) throw new Error('--orbit and --slide both read --step: give one of them');
  if ((orbit > 0 || slide > 0) && reproject) renderer.setMeanByCount(true);
  renderer.resize(width, height);
  const t0 = Date.now();
  let until = null;
  if (untilArg !== null) {
    const checkEvery = arg('check-every', null);
    until = renderer.renderUntil(scene, camera, parseFloat(untilArg), { maxFrames: frames, minFrames: parseInt(arg('min-frames', '16'), 10),
      checkEvery: checkEvery === null ? undefined : parseInt(checkEvery, 10), lookahead: !process.argv.includes('--no-lookahead'),
      adaptive: process.argv.includes('--adaptive'), guard: parseInt(arg('guard', '1'), 10) });
    renderer.render(scene, camera);                                        // only presents
    console.error('--until ' + untilArg + ': ' + (until.converged ? 'converged' : 'not converged') + ' after ' + until.frames + ' of ' + frames + ' frames');
  } else if (orbit > 0) {
    const spp = parseInt(arg('spp', '4'), 10), step = parseFloat(arg('step', '2')) * Math.PI / 180;
    const p0 = camera.position.clone();
    renderer.frames = spp;
    for (let view = 0; view < orbit; view++) {
      const c = Math.cos(view * step), s = Math.sin(view * step);
      camera.position.copy(new pt.Vector3(c * p0.x + s * p0.z, p0.y, -s * p0.x + c * p0.z));
      camera.lookAt(0, 0, 0);
      let held = null;
      if (view > 0) {
        if (reproject) held = hold(renderer.reproject(scene, camera));
        else renderer.reset();
      }
      sample(spp, held, 'view ' + view);
      fs.writeFileSync(out + '_view' + view + '.acc.f32', Buffer.from(renderer.readAccumulation().buffer));
      fs.writeFileSync(out + '_view' + view + '.uniforms.bin', Buffer.from(renderer.passes.raytrace.uniforms.bytes));
      if (guidedVariance) renderer.denoiseGuided({ variance: true, present: true, despike, young });
      renderer.screenshot(out + '_view' + view + '.png');
    }
  } else if (slide > 0) {
    const spp = parseInt(arg('spp', '4'), 10), step = parseFloat(arg('step', '0.1'));
    const box = scene.children.find((c) => c instanceof pt.Mesh && c.geometry instanceof pt.BoxGeometry);
    if (!box) throw new Error('--slide moves the box of the default scene');
    const x0 = box.position.x;
    renderer.frames = spp;
    for (let k = 0; k < slide; k++) {
      let held = null;
      if (k > 0) {
        box.position.x = x0 + k * step;
        scene.needsUpdate = true;
        if (reproject) held = hold(renderer.reprojectScene(scene, camera));
        else renderer.reset();
      }
      sample(spp, held, 'step ' + k);
      if (refit) {
        const ratio = renderer.lastRefitCostRatio;
        refitRatios.push(ratio);
        console.error('--refit: step ' + k + ': ' + (ratio === null ? 'built on the host' : 'cost ratio ' + ratio.toFixed(4) + ', ' + renderer.lastRefitMs.toFixed(3) + ' ms on the device'));
        fs.writeFileSync(out + '_step' + k + '.nodes.bin', renderer.passes.raytrace.nodeBytes);
      }
      fs.writeFileSync(out + '_step' + k + '.acc.f32', Buffer.from(renderer.readAccumulation().buffer));
      fs.writeFileSync(out + '_step' + k + '.uniforms.bin', Buffer.from(renderer.passes.raytrace.uniforms.bytes));
      renderer.screenshot(out + '_step' + k + '.png');
    }
  } else {
    for (let i = 0; i < frames + 1; i++) renderer.render(scene, camera);   // the last call only presents
  }
  const firstStats = renderer.passes.raytrace.stats;
  if (process.argv.includes('--second-scene')) {
    scene.remove(scene.children[scene.children.length - 1]);
    scene.needsUpdate = true;
    renderer.reset();
    for (let i = 0; i < frames + 1; i++) renderer.render(scene, camera);
  }
  const acc = renderer.readAccumulation();
  const ms = Date.now() - t0;
  const canvas = renderer.readCanvas();
  fs.writeFileSync(out + '.acc.f32', Buffer.from(acc.buffer));
  fs.writeFileSync(out + '.canvas.rgba8', Buffer.from(canvas.buffer));
  renderer.screenshot(out + '.png');
  if (process.argv.includes('--aovs')) {
    renderer.renderAovs(['albedo', 'normal', 'position']);
    const toPng = (img, fn) => {                     // rows flipped: the canvas has row 0 at the top
      const px = new Uint8Array(width * height * 4);
      for (let y = 0; y < height; y++) {
        for (let x = 0; x < width; x++) {
          const s = ((height - 1 - y) * width + x) * 4, d = (y * width + x) * 4;
          for (let c = 0; c < 3; c++) px[d + c] = Math.max(0, Math.min(255, Math.round(255 * fn(img[s + c], img, s))));
          px[d + 3] = 255;
        }
      }
      return pt.encodePNG(px, width, height);
    };
    const normal = renderer.readAov('normal');
    fs.writeFileSync(out + '_albedo.png', toPng(renderer.readAov('albedo'), (v) => v));
    fs.writeFileSync(out + '_normal.png', toPng(normal, (v, img, s) => (img[s] === 0 && img[s + 1] === 0 && img[s + 2] === 0 ? 0 : 0.5 * v + 0.5)));
    fs.writeFileSync(out + '_position.f32', Buffer.from(renderer.readAov('position').buffer));
  }
  if (process.argv.includes('--guided')) {
    renderer.denoiseGuided({ present: true, despike });
    if (despike) sayDespiked();
    fs.writeFileSync(out + '_guided.f32', Buffer.from(renderer.readGuided().buffer));
    renderer.screenshot(out + '_guided.png');
  }
  if (guidedVariance) {
    renderer.denoiseGuided({ variance: true, present: true, despike, young });
    if (despike) sayDespiked();
    fs.writeFileSync(out + '_guided.f32', Buffer.from(renderer.readGuided().buffer));
    fs.writeFileSync(out + '_guided_variance.f32', Buffer.from(renderer.readGuidedVariance().buffer));
    fs.writeFileSync(out + '_moments.f32', Buffer.from(renderer.readMoments().buffer));
    renderer.screenshot(out + '_guided.png');
  }
  if (untilArg !== null && process.argv.includes('--adaptive')) {
    fs.writeFileSync(out + '_mask.u8', Buffer.from(renderer.readSampleMask()));
    fs.writeFileSync(out + '_moments.f32', Buffer.from(renderer.readMoments().buffer));
  }
  const summary = {
    width, height, frames, until, despiked, validate: validate > 0 ? { frames: validate, kept: keptShares } : undefined, refit: refit ? refitRatios : undefined, status: renderer.status, frame: renderer.frame, events,
    counters: renderer.counters(), stats: renderer.passes.raytrace.stats, first_stats: firstStats, wall_ms: ms,
    timings_us: { raytrace: renderer.timings.raytrace.value, accumulate: renderer.timings.accumulate.value,
      fullscreen: renderer.timings.fullscreen.value },
    device: diag.info.description,
  };
  console.log(JSON.stringify(summary));
  await renderer.destroy();
}

main().catch((err) => { console.error(err.stack || String(err)); process.exit(1); });
