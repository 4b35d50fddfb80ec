------------------------------- MODULE beyond --------------------------------
(* For mc_engine_behaviours: a CONSTRAINT bounds the search, not the system.  The counter grows for ever and the cfg checks it up to
   x <= 2; an implementation that logged x = 0, 1, 2, 3, 4 still ran a behaviour of this spec.  It is accepted, and the two steps
   that leave the constraint are counted (outside = 2). *)
EXTENDS Naturals
(* --algorithm beyond
variables x = 0;
define
  Small == x <= 2
end define;
process P = 0
begin
  s: while TRUE do
       x := x + 1;
     end while;
end process

end algorithm *)
=============================================================================
